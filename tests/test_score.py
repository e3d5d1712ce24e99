"""Transcript likelihood (score / score_batch) on the CPU simulator of the kernels, which runs the body of ctc_forward
(csrc/ctc_align.h) itself with a one-thread context: every shape case of tests/align_util.py and the cases of
tests/score_util.py against the numpy forward recursion, the single-path cases against align, the probabilities of all label
sequences summing to 1, batches equal to single calls float for float, the language-model term against the beam search's own,
and the refusals of the Python surface and of the C entry point. The HIP build: tests/test_gpu_score.py."""
import math
import os

import numpy as np
import pytest

from tests.score_util import (NORMALISATION, SCORE_TOL, SINGLE_PATH, all_sequences, case_input, feasible, neg_inf_case,
                              normalisation_input, random_logits, random_target, shape_cases, yardstick)
from tests.sim_util import sim_library  # noqa: F401
from tests.test_align import build, ragged_batch

SHAPES = shape_cases()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check_score(got, want, what):
    print("%s: score %.12f, numpy %.12f" % (what, got, want))
    if math.isinf(want):
        assert got == want, (what, got, want)
    else:
        assert abs(got - want) <= SCORE_TOL, (what, got, want, got - want)


def ragged_hyps(targets, V=29, seed=9):
    """Per utterance of ragged_batch(): its own target, a longer and a shorter variant, one with a label substituted -- and
    for every third utterance one too long to align."""
    rng = np.random.default_rng(seed)
    out = []
    for u, t in enumerate(targets):
        hyps = [list(t), list(t) + random_target(rng, 2, V), list(t[:-1])]
        if t:
            sub = list(t)
            sub[int(rng.integers(0, len(t)))] = int(rng.integers(2, V))
            hyps.append(sub)
        if u % 3 == 0:
            hyps.append(random_target(rng, 70, V))
        out.append(hyps)
    return out


@pytest.mark.parametrize("case", SHAPES, ids=[c[0] for c in SHAPES])
def test_shape_cases(case, sim_library):  # noqa: F811
    name, V, T, target, _dtype, _kind = case
    dec = build(V)
    x = case_input(case)
    blank = dec._alphabet.labels.index("")
    got = dec.score(x, tokens=[target])
    assert len(got) == 1 and got[0].tokens == list(target) and got[0].lm_logp is None and got[0].total == got[0].logp
    check_score(got[0].logp, yardstick(x, target, blank), name)
    assert sum(dec.last_score_launched) == (1 if T > 0 else 0)
    if T == 0:
        assert got[0].logp == 0.0
        return
    best = dec.align(x, tokens=target).score
    print("%s: best path %.12f" % (name, best))
    if name in SINGLE_PATH:
        assert abs(got[0].logp - best) <= SCORE_TOL, (name, got[0].logp, best)
    else:
        assert got[0].logp > best, (name, got[0].logp, best)


def test_no_frames_and_neg_inf_logits(sim_library):  # noqa: F811
    dec = build(29)
    blank = dec._alphabet.labels.index("")
    empty = np.zeros((0, 29))
    got = dec.score(empty, tokens=[[2, 3], []])
    assert got[0].logp == -np.inf and got[1].logp == 0.0 and dec.last_score_launched == (0, 0)
    x, target = neg_inf_case()
    assert np.isneginf(x[:, target]).any()
    got = dec.score(x, tokens=[target])[0].logp
    assert math.isfinite(got)
    check_score(got, yardstick(x, target, blank), "-inf logits")


@pytest.mark.parametrize("V,T,n_hyps,n_infeasible", NORMALISATION, ids=["V%d_T%d" % c[:2] for c in NORMALISATION])
def test_all_sequences_sum_to_one(V, T, n_hyps, n_infeasible, sim_library):  # noqa: F811
    dec = build(V)
    blank = dec._alphabet.labels.index("")
    x = normalisation_input(V, T)
    seqs = all_sequences(V, T, blank)
    assert len(seqs) == n_hyps and sum(1 for s in seqs if not feasible(T, s)) == n_infeasible
    got = dec.score(x, tokens=seqs)
    for s, g in zip(seqs, got):
        if feasible(T, s):
            check_score(g.logp, yardstick(x, s, blank), str(s))
        else:
            assert g.logp == -np.inf, (s, g.logp)
    total = math.fsum(math.exp(g.logp) for g in got)
    print("V=%d T=%d: the probabilities of %d sequences sum to 1 %+.3e" % (V, T, n_hyps, total - 1.0))
    assert abs(total - 1.0) <= 1e-12, total
    assert sum(dec.last_score_launched) == n_hyps - n_infeasible


def test_batch_equals_single_calls(sim_library):  # noqa: F811
    dec = build(29)
    blank = dec._alphabet.labels.index("")
    xs, targets = ragged_batch()
    hyps = ragged_hyps(targets)
    batch = dec.score_batch(xs, tokens=hyps)
    singles = [dec.score(x, tokens=h) for x, h in zip(xs, hyps)]
    for u, (x, h) in enumerate(zip(xs, hyps)):
        assert [g.logp for g in batch[u]] == [g.logp for g in singles[u]], u
        for t, g in zip(h, batch[u]):
            check_score(g.logp, yardstick(x, t, blank), "utt %d" % u)
            assert g.tokens == t
    # padded into one [B, T, V] array: every row of an utterance is a frame -- equal to the single calls on the padded matrices
    T = max(len(x) for x in xs)
    pad = np.zeros((len(xs), T, 29))
    for u, x in enumerate(xs):
        pad[u, : len(x)] = x
    cube = dec.score_batch(pad, tokens=hyps)
    for u, h in enumerate(hyps):
        assert [g.logp for g in cube[u]] == [g.logp for g in dec.score(pad[u], tokens=h)], u
        check_score(cube[u][0].logp, yardstick(pad[u], h[0], blank), "padded %d" % u)
    # the hypotheses of an utterance in another order
    rng = np.random.default_rng(2)
    perms = [rng.permutation(len(h)).tolist() for h in hyps]
    shuffled = dec.score_batch(xs, tokens=[[h[k] for k in p] for h, p in zip(hyps, perms)])
    for u, p in enumerate(perms):
        assert [g.logp for g in shuffled[u]] == [batch[u][k].logp for k in p], u


def test_utterances_that_launch_nothing_and_lazy_inputs(sim_library):  # noqa: F811
    """An utterance without hypotheses, or with none that has an alignment, takes no part in the device work and changes
    nobody's floats; hypotheses may come from generators; the diagnostics exist from the start and follow an empty call."""
    dec = build(29)
    assert dec.last_score_launched == (0, 0) and dec.last_score_timing_ms == (0.0, 0.0, 0.0, 0.0)
    rng = np.random.default_rng(12)
    xs = [random_logits(rng, T, 29) for T in (30, 12, 5, 20)]
    t = random_target(rng, 7, 29)
    hyps = [[t, t[:3]], [], [random_target(rng, 9, 29)], [t[1:]]]
    got = dec.score_batch(xs, tokens=hyps)
    assert dec.last_score_launched == (3, 0) and got[1] == [] and got[2][0].logp == -np.inf
    for u in (0, 3):
        assert [g.logp for g in got[u]] == [g.logp for g in dec.score(xs[u], tokens=hyps[u])]
    lazy = dec.score_batch(iter(xs), tokens=(iter(h) for h in hyps))
    assert [[g.logp for g in a] for a in lazy] == [[g.logp for g in a] for a in got]
    assert dec.score_batch([], []) == [] and dec.last_score_launched == (0, 0)


def test_text_and_tokens_give_the_same_float(sim_library):  # noqa: F811
    dec = build(29)
    labels = dec._alphabet.labels
    x = random_logits(np.random.default_rng(8), 40, 29)
    texts = ["  bugs   bunny \n", "bug", ""]
    toks = [[labels.index(c) for c in " ".join(t.split())] for t in texts]
    a, b = dec.score(x, texts), dec.score(x, tokens=toks)
    assert [g.logp for g in a] == [g.logp for g in b] and [g.tokens for g in a] == toks
    assert [g.text for g in a] == ["bugs bunny", "bug", ""] == [g.text for g in b]
    assert a[0].logp == dec.score_batch([x, x], [["bug"], ["bugs bunny"]])[1][0].logp


@pytest.fixture(scope="module")
def lm():
    import synth

    return synth.SynthLM(os.path.join(ROOT, "tests", "golden", "_lm"), 300, 400, order=4, seed=2)


def test_with_lm_is_the_beam_searchs_term(lm, sim_library):  # noqa: F811
    import synth
    from pyctcdecode_amd import build_ctcdecoder

    dec = build_ctcdecoder(synth.LIBRI_LABELS, lm.path)
    n, worst = 0, 0.0
    for seed in range(4):
        x = synth.d_words(2, seed, 80, synth.LIBRI_LABELS, False, lm.words, lm.sentences, 28, boost=2.5).astype(np.float64)
        beams = dec.decode_beams(x, beam_width=50)
        got = dec.score(x, [b.text for b in beams], with_lm=True)
        for b, g in zip(beams, got):
            gap = abs(g.lm_logp - (b.lm_score - b.logit_score))
            worst = max(worst, gap)
            assert gap <= 1e-9, (seed, b.text, g.lm_logp, b.lm_score - b.logit_score)
            assert g.total == g.logp + g.lm_logp and g.text == b.text
            n += 1
    print("with_lm: %d beams, worst gap %.1e" % (n, worst))
    assert n >= 8
    with pytest.raises(ValueError, match="language model"):
        build(29).score(np.zeros((5, 29)), ["a"], with_lm=True)


def test_bad_arguments(sim_library):  # noqa: F811
    from pyctcdecode_amd import build_ctcdecoder

    dec = build(5)
    labels = dec._alphabet.labels
    x = np.zeros((9, 5))
    with pytest.raises(ValueError, match="utterance 0.*bare str"):
        dec.score(x, "ab")
    with pytest.raises(ValueError, match="utterance 1.*bare str"):
        dec.score_batch([x, x], [["ab"], "ab"])
    with pytest.raises(ValueError, match="2 utterances"):
        dec.score_batch([x, x], [["a"]])
    with pytest.raises(ValueError, match="utterances"):
        dec.score_batch([x], "a")
    for bad in ([labels.index("")], [5], [-1], [2.0], [True]):
        with pytest.raises(ValueError, match="utterance 0, hypothesis 1.*label id"):
            dec.score(x, tokens=[[2], bad])
    with pytest.raises(ValueError, match="utterance 0, hypothesis 0.*limit of 2047"):
        dec.score(np.zeros((2100, 5)), tokens=[random_target(np.random.default_rng(1), 2048, 5)])
    with pytest.raises(ValueError, match="'z'"):
        dec.score(x, ["ab z"])
    with pytest.raises(ValueError, match="exactly one"):
        dec.score(x, ["ab"], tokens=[[2, 3]])
    with pytest.raises(ValueError, match="exactly one"):
        dec.score_batch([x])
    with pytest.raises(ValueError):
        dec.score(np.zeros((9, 6)), ["ab"])
    assert dec.score_batch([], []) == [] and dec.score(x, []) == []
    bpe = build_ctcdecoder(["<unk>", "▁bug", "s", "▁bun", "ny", "▁", "n", "▁a"])
    xb = random_logits(np.random.default_rng(4), 25, len(bpe._alphabet.labels))
    with pytest.raises(ValueError, match="tokens="):
        bpe.score(xb, ["bugs bunny"])
    lab = bpe._alphabet.labels
    target = [lab.index(p) for p in ("▁bug", "s", "▁bun", "n", "n", "ny", "▁a")]
    got = bpe.score(xb, tokens=[target])[0]
    assert got.text == "bugs bunnnny a"
    check_score(got.logp, yardstick(xb, target, lab.index("")), "bpe")


def test_native_call_validates_what_it_indexes_with(sim_library):  # noqa: F811
    """The C entry point on its own: null pointers, decreasing offsets, a label outside the alphabet, the blank and too many
    labels are error codes before anything is launched, and the process lives."""
    import ctypes as C

    dec = build(5)
    blank = dec._alphabet.labels.index("")
    x = np.zeros((4, 5))
    I32, I64, F64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)

    def call(targets, toff=None, hoff=None, frames=4, null=(), kernel=0):
        ptrs = (C.c_void_p * 1)(None if "x" in null else x.ctypes.data)
        fr = (C.c_int32 * 1)(frames)
        flat = np.array([c for t in targets for c in t] or [0], dtype=np.int32)
        to = np.array(toff if toff is not None else np.concatenate(([0], np.cumsum([len(t) for t in targets]))), dtype=np.int64)
        ho = np.array(hoff if hoff is not None else [0, len(targets)], dtype=np.int64)
        out = np.full(max(len(targets), 1), 7.0)
        ms, launched = (C.c_double * 4)(), (C.c_int64 * 2)()
        rc = dec._lib.dll.ctcdec_score_batch(
            None if "dec" in null else dec._handle, None if "ptrs" in null else ptrs, None if "frames" in null else fr, 1, 1, 0,
            None if "targets" in null else flat.ctypes.data_as(I32), None if "toff" in null else to.ctypes.data_as(I64),
            None if "hoff" in null else ho.ctypes.data_as(I64), kernel, None if "out" in null else out.ctypes.data_as(F64),
            None if "diag" in null else ms, None if "diag" in null else launched)
        return rc, out.tolist()

    rc, out = call([[2, 3], [2, 2, 2], []])
    assert rc == 0 and math.isfinite(out[0]) and out[1] == -np.inf and math.isfinite(out[2])
    assert call([[2, 3]], null=("diag",)) == (rc, out[:1])
    for what in ("dec", "ptrs", "frames", "targets", "toff", "hoff", "out", "x"):
        assert call([[2, 3]], null=(what,))[0] == -1, what
    assert call([[2, 5]])[0] == -1 and call([[2], [-1]])[0] == -1 and call([[blank]])[0] == -1
    assert call([[2, 3]], toff=[0, -1])[0] == -1 and call([[2, 3]], toff=[1, 2])[0] == -1
    assert call([[2], [3]], toff=[0, 2, 1])[0] == -1
    assert call([[2, 3]], hoff=[0, -1])[0] == -1 and call([[2, 3]], hoff=[1, 1])[0] == -1
    assert call([[2, 3]], frames=-1)[0] == -1 and call([[2, 3]], kernel=3)[0] == -1
    assert call([[2] * 2048])[0] == -4
    assert call([[2, 3]])[0] == 0  # (the decoder still works)


def test_parallel_refuses(sim_library):  # noqa: F811
    from pyctcdecode_amd.parallel import DevicePool, score_batch_sharded

    dec = build(5)
    with pytest.raises(NotImplementedError):
        score_batch_sharded(dec, [np.zeros((3, 5))], [["a"]])
    with DevicePool(dec, devices=[0], library=sim_library.path) as pool:
        with pytest.raises(NotImplementedError):
            pool.score_batch([np.zeros((3, 5))], [["a"]])
        with pytest.raises(NotImplementedError):
            pool.score(np.zeros((3, 5)), ["a"])
