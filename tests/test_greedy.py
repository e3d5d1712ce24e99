"""Greedy best-path decoding (decode_greedy / decode_greedy_batch) on the CPU simulator of the kernels, which runs the bodies
of csrc/ctc_align.h themselves with a one-lane context: the row labels under ties, signed zeros, NaN and -inf, the collapse
around the 64-frame step, the native text against _words_of_target for both alphabet kinds, the exact identities with align
and align_gaps, batches against single calls, the cost contract and the refusals. The HIP build: tests/test_gpu_greedy.py,
which runs the same cases through the run_* functions here."""
import ctypes as C

import numpy as np
import pytest

from tests.align_gaps_util import items_of
from tests.align_util import random_logits, spans_of
from tests.greedy_util import (BLANK, SPACE, VOCABS, argmax_np, build, check_greedy, collapse_np, collapse_sequences,
                               logits_of_labels, of_batch, probability_rows, same_batch_entry, special_rows, tie_rows,
                               unique_maxima)
from tests.sim_util import sim_library  # noqa: F401
from tests.token_logp_util import FOLDS

HOST_DTYPES = (np.float16, np.float32, np.float64)
SEQS = collapse_sequences()
IDENTITY_SEEDS = {29: 3, 131: 4, 300: 5, 1024: 6}  # (test_identity_premise_holds_for_every_seed checks them here, on the CPU)


def same(x):
    return x


def tokens_of_rows(want):
    return [c for c, _, _ in collapse_np(want, BLANK)]


# ---- the cases, for host arrays (here) and through `put` for device tensors (tests/test_gpu_greedy.py) ------------------------
def run_ties(V, dtype, put=same):
    """The answer is always the smaller index, whichever lane folds which entry; +0.0 and -0.0 are one value."""
    dec = build(V)
    x, want = tie_rows(V, np.dtype(dtype).itemsize, np.random.default_rng(V))
    xt = x.astype(dtype)
    assert np.array_equal(argmax_np(xt, BLANK), want)  # (the yardstick itself)
    plain = dec.decode_greedy(put(xt), token_frames=True)
    conf = dec.decode_greedy(put(xt), confidence="min")
    assert plain.tokens == tokens_of_rows(want), (V, dtype, plain.tokens)
    assert [s for _l, (s, _e) in plain.token_frames] == [t for t, c in enumerate(want) if c not in (BLANK, SPACE)]
    check_greedy(plain, xt, dec, None, "ties V=%d %s" % (V, np.dtype(dtype)))
    check_greedy(conf, xt, dec, "min", "ties V=%d %s conf" % (V, np.dtype(dtype)))
    assert conf.tokens == plain.tokens and conf.token_frames == plain.token_frames  # row_lse_argmax's label is row_argmax's
    return plain, conf


def run_special_rows(V, put=same):
    dec = build(V)
    x, want = special_rows(V, np.random.default_rng(V + 1))
    assert np.array_equal(argmax_np(x, BLANK), want)
    out = []
    for dtype in HOST_DTYPES:
        xt = x.astype(dtype)
        plain = dec.decode_greedy(put(xt), token_frames=True)
        assert plain.tokens == tokens_of_rows(want), (V, dtype)
        check_greedy(plain, xt, dec, None, "special V=%d" % V)
        for fold in FOLDS:
            conf = dec.decode_greedy(put(xt), confidence=fold)
            check_greedy(conf, xt, dec, fold, "special V=%d %s %s" % (V, np.dtype(dtype), fold))  # (a finite score: the floor)
            assert conf.tokens == plain.tokens and conf.token_frames == plain.token_frames
            out.append(conf)
        out.append(plain)
    return out


def run_collapse(name, put=same, V=29):
    dec = build(V)
    seq = SEQS[name]
    x = logits_of_labels(seq, V, np.random.default_rng(len(name)))
    plain = dec.decode_greedy(put(x), token_frames=True)
    conf = dec.decode_greedy(put(x), confidence="mean")
    want = collapse_np(np.asarray(seq, dtype=np.int32), BLANK)
    assert plain.tokens == [c for c, _, _ in want] and [f for _l, f in plain.token_frames] == [(s, e) for _c, s, e in want], name
    check_greedy(plain, x, dec, None, name)
    check_greedy(conf, x, dec, "mean", name)
    assert dec.decode_greedy(put(x)) == plain.text
    return plain, conf


def ragged_inputs(V=29, dtype=np.float64):
    """Utterances of 0 and 1 frames between long ones (the scan of the counts), every collapse sequence among them."""
    rng = np.random.default_rng(77)
    xs = []
    for k, name in enumerate(sorted(SEQS)):
        xs.append(logits_of_labels(SEQS[name], V, rng, dtype))
        if k % 5 == 0:
            xs.append(np.zeros((0, V), dtype=dtype))
            xs.append(logits_of_labels([9], V, rng, dtype))
    xs.append(random_logits(rng, 200, V).astype(dtype))
    xs.append(np.zeros((0, V), dtype=dtype))
    return xs


def run_batch_equals_single_calls(put=same, fold="mean", xs=None, V=29):
    dec = build(V)
    xs = ragged_inputs(V) if xs is None else xs
    xin = [put(x) for x in xs]
    texts, frames = dec.decode_greedy_batch(xin, confidence=fold) if fold else dec.decode_greedy_batch(xin, token_frames=True)
    assert dec.decode_greedy_batch(xin) == texts
    assert len(frames) == len(xs) and (frames.score is None) == (fold is None)
    singles = []
    for u, x in enumerate(xs):
        g = dec.decode_greedy(xin[u], token_frames=True, confidence=fold)
        check_greedy(g, x, dec, fold, "utt %d" % u)
        assert same_batch_entry(of_batch(texts, frames, u, dec), g), u
        singles.append(g)
    return dec, xs, xin, texts, frames, singles


def mixed_inputs(V, dtype):
    """Probability utterances (powers of two: exact in every dtype) in one batch with logit utterances."""
    rng = np.random.default_rng(V + 7)
    p = probability_rows(33, V, rng).astype(dtype)
    return [p, random_logits(rng, 40, V).astype(dtype), p[:7].copy(), random_logits(rng, 65, V).astype(dtype)]


def identity_input(V, dtype=np.float64):
    return random_logits(np.random.default_rng(IDENTITY_SEEDS[V]), 70, V).astype(dtype)


def run_family_identities(V, dtype, put=same):
    """The greedy path is a path of its own labels and no path beats the frames' maxima: align and the all-gap align_gaps give
    the greedy score exactly; where the maxima are unique, align's path is the greedy path."""
    dec = build(V)
    x = identity_input(V, dtype)
    unique = np.dtype(dtype) == np.float64
    if unique:
        assert unique_maxima(x), V  # (asserted, never a reason to skip: the seeds are chosen so that it holds)
    else:
        x = np.round(x).astype(dtype)  # (small integers: ties in most rows)
        assert not unique_maxima(x)
    xin = put(x)
    out = []
    for fold in FOLDS:
        g = dec.decode_greedy(xin, confidence=fold)
        check_greedy(g, x, dec, fold, "identity V=%d %s %s" % (V, np.dtype(dtype), fold))
        assert len(g.tokens) >= 1
        a = dec.align(xin, tokens=g.tokens, confidence=fold)
        gaps = dec.align_gaps(xin, tokens=items_of(g.tokens, [1] * (len(g.tokens) + 1)))
        print("V=%d %s %s: greedy %.17g align %.17g all-gap %.17g" % (V, np.dtype(dtype), fold, g.score, a.score, gaps.score))
        assert g.score == a.score and g.score == gaps.score
        if unique:
            runs = spans_of(a.path, BLANK)
            assert [c for c, _, _ in runs] == g.tokens
            assert a.token_frames == g.token_frames and a.text_frames == g.text_frames and a.text == g.text
            assert a.token_logp == g.token_logp and a.word_logp == g.word_logp
            assert np.array_equal(a.path, argmax_np(x, BLANK))
        out.append(g)
    return out


def char_text_case(V=29):
    """Greedy labels with a leading, a trailing and a doubled space label (two space tokens: a blank frame between them)."""
    a, b, c = 4, 9, 20
    seq = [SPACE, SPACE, a, a, b, BLANK, b, SPACE, BLANK, SPACE, c, BLANK, SPACE]
    return seq, logits_of_labels(seq, V, np.random.default_rng(8))


BPE_PIECES = ["<unk>", "▁bug", "s", "▁bun", "ny", "▁", "n", "▁a", "er▁", "▁x▁"]


def bpe_text_case():
    from pyctcdecode_amd import build_ctcdecoder

    dec = build_ctcdecoder(BPE_PIECES)
    labels = dec._alphabet.labels
    assert dec._alphabet.is_bpe
    blank = labels.index("")
    order = ("▁", "▁bug", "s", "er▁", "n", "ny", "▁", "▁", "▁x▁", "s", "▁bun", "ny", "▁a", "er▁")
    seq = []
    for k, piece in enumerate(order):
        seq += [labels.index(piece)] * (1 + k % 3) + ([blank] if k % 2 or piece == "▁" else [])
    x = logits_of_labels(seq, len(labels), np.random.default_rng(9))
    return dec, seq, x


def run_texts(put=same):
    out = []
    dec = build(29)
    seq, x = char_text_case()
    g = dec.decode_greedy(put(x), confidence="max")
    lab = dec._alphabet.labels
    assert g.tokens == [SPACE, 4, 9, 9, SPACE, SPACE, 20, SPACE] and g.text == lab[4] + lab[9] + lab[9] + " " + lab[20]
    out.append((dec, x, g))
    bdec, bseq, bx = bpe_text_case()
    g = bdec.decode_greedy(put(bx), confidence="max")
    assert g.tokens == [c for c, _, _ in collapse_np(np.asarray(bseq), bdec._alphabet.labels.index(""))]
    assert [w for w, _ in g.text_frames] == ["", "bugser", "nny", "", "", "x", "s", "bunny", "aer"], g.text_frames
    out.append((bdec, bx, g))
    for d, xx, g in out:
        check_greedy(g, xx, d, "max", "text")
        text, kept, _words = d._words_of_target(g.tokens)
        texts, frames = d.decode_greedy_batch([put(xx), put(xx[:3])], token_frames=True)
        assert texts[0] == text == g.text and frames.of(0) == g.token_frames  # (the batch's text is the native one, as it came)
        a = d.align(put(xx), tokens=g.tokens, confidence="max")
        assert a.text == g.text and a.text_frames == g.text_frames and a.token_frames == g.token_frames
        assert a.word_logp == g.word_logp and a.score == g.score
    return [g for _d, _x, g in out]


# ---- the simulator -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("dtype", HOST_DTYPES, ids=lambda d: np.dtype(d).name)
def test_ties_take_the_smaller_index(sim_library, dtype, V):  # noqa: F811
    run_ties(V, dtype)


@pytest.mark.parametrize("V", (29, 131))
def test_nan_and_inf_rows(sim_library, V):  # noqa: F811
    run_special_rows(V)


@pytest.mark.parametrize("name", sorted(SEQS))
def test_collapse(sim_library, name):  # noqa: F811
    run_collapse(name)


def test_empty_utterance_and_empty_batch(sim_library):  # noqa: F811
    dec = build(29)
    empty = np.zeros((0, 29))
    assert dec.decode_greedy(empty) == ""
    g = dec.decode_greedy(empty, confidence="mean")
    assert g.text == "" and g.tokens == [] and g.token_frames == [] and g.token_logp == [] and g.score == 0.0
    assert dec.last_greedy_launches == 0
    assert dec.decode_greedy_batch([]) == []
    texts, frames = dec.decode_greedy_batch([], confidence="mean")
    assert texts == [] and len(frames) == 0 and len(frames.label) == 0 and len(frames.score) == 0 and len(frames.logp) == 0
    texts, frames = dec.decode_greedy_batch([], token_frames=True)
    assert texts == [] and frames.score is None and frames.logp is None


@pytest.mark.parametrize("fold", (None, "mean"))
def test_ragged_batch_equals_single_calls(sim_library, fold):  # noqa: F811
    dec, xs, _xin, texts, frames, singles = run_batch_equals_single_calls(fold=fold)
    assert frames.offsets[-1] == sum(len(g.token_frames) for g in singles) > 300
    assert any(len(x) == 0 for x in xs) and any(len(x) == 1 for x in xs)


def test_batch_as_a_cube(sim_library):  # noqa: F811
    dec = build(29)
    rng = np.random.default_rng(2)
    cube = random_logits(rng, 3 * 41, 29).reshape(3, 41, 29)
    texts, frames = dec.decode_greedy_batch(cube, confidence="min")
    for u in range(3):
        g = dec.decode_greedy(cube[u], confidence="min")
        check_greedy(g, cube[u], dec, "min", "cube %d" % u)
        assert same_batch_entry(of_batch(texts, frames, u, dec), g)


@pytest.mark.parametrize("dtype", HOST_DTYPES, ids=lambda d: np.dtype(d).name)
def test_probabilities_and_logits_in_one_batch(sim_library, dtype):  # noqa: F811
    xs = mixed_inputs(29, dtype)
    run_batch_equals_single_calls(fold="mean", xs=xs)
    run_batch_equals_single_calls(fold=None, xs=xs)


def test_texts_of_both_alphabet_kinds(sim_library):  # noqa: F811
    run_texts()


def test_identity_premise_holds_for_every_seed():
    for V in VOCABS:
        assert unique_maxima(identity_input(V)), V


@pytest.mark.parametrize("V", VOCABS)
def test_family_identities(sim_library, V):  # noqa: F811
    run_family_identities(V, np.float64)


@pytest.mark.parametrize("V", (29, 131))
def test_score_identity_under_ties(sim_library, V):  # noqa: F811
    run_family_identities(V, np.float16)


def test_greedy_frames_pickle_and_join(sim_library):  # noqa: F811
    import pickle

    from pyctcdecode_amd import GreedyFrames, TokenFrames

    dec = build(29)
    xs = mixed_inputs(29, np.float32)
    _t, a = dec.decode_greedy_batch(xs[:2], confidence="mean")
    _t, b = dec.decode_greedy_batch(xs[2:], confidence="mean")
    _t, whole = dec.decode_greedy_batch(xs, confidence="mean")
    assert isinstance(whole, TokenFrames) and not hasattr(whole, "__dict__")
    joined = GreedyFrames.join([a, b], dec._alphabet.labels)
    again = pickle.loads(pickle.dumps(whole))
    for other in (joined, again):
        assert type(other) is GreedyFrames
        for name in ("label", "start", "end", "offsets", "logp", "score"):
            assert np.array_equal(getattr(other, name), getattr(whole, name)), name
        assert other.labels == whole.labels


def test_cost_contract(sim_library):  # noqa: F811
    """A plain call classifies nothing and forms no log-sum-exp: three launches (row_argmax, greedy_collapse's two passes), no
    prune stage. (The simulator takes no kernel times: tests/test_gpu_greedy.py holds the confidence call's against 0.)"""
    dec = build(29)
    x = random_logits(np.random.default_rng(1), 30, 29)
    dec.decode_greedy(x)
    assert dec.last_greedy_launches == 3
    assert dec.last_greedy_timing_ms[0] == 0.0 and dec.last_greedy_lse_ms == 0.0 and dec.last_greedy_timing_ms[3] > 0.0
    dec.decode_greedy(x, confidence="mean")
    assert dec.last_greedy_launches == 3 and len(dec.last_greedy_timing_ms) == 4


def test_refusals(sim_library):  # noqa: F811
    from pyctcdecode_amd import _binding as B
    from pyctcdecode_amd.parallel import DevicePool

    dec = build(29)
    x = random_logits(np.random.default_rng(1), 10, 29)
    for bad in ("median", 2, True):
        with pytest.raises(ValueError, match="confidence"):
            dec.decode_greedy(x, confidence=bad)
        with pytest.raises(ValueError, match="confidence"):
            dec.decode_greedy_batch([x], confidence=bad)
    for wrong in (x[0], random_logits(np.random.default_rng(1), 10, 30)):
        with pytest.raises(ValueError):
            dec.decode_greedy(wrong)
        with pytest.raises(ValueError):
            dec.decode_greedy_batch([x, wrong])
    pool = object.__new__(DevicePool)  # (no workers started: the refusal comes first)
    with pytest.raises(NotImplementedError):
        pool.decode_greedy_batch([x])
    with pytest.raises(NotImplementedError):
        dec.decode_greedy_batch(pool)
    # the C entry point: CTCDEC_ERR_ARG before anything moves
    dll, h = sim_library.dll, dec._handle
    ptrs = np.ascontiguousarray([x.ctypes.data], dtype=np.uint64)
    frames = np.ascontiguousarray([10], dtype=np.int32)
    pp, fp = ptrs.ctypes.data_as(C.POINTER(C.c_void_p)), frames.ctypes.data_as(C.POINTER(C.c_int32))
    res = C.c_void_p()
    assert dll.ctcdec_greedy_batch(None, pp, fp, 1, 1, 0, 0, C.byref(res)) == -1
    assert dll.ctcdec_greedy_batch(h, None, fp, 1, 1, 0, 0, C.byref(res)) == -1
    assert dll.ctcdec_greedy_batch(h, pp, None, 1, 1, 0, 0, C.byref(res)) == -1
    assert dll.ctcdec_greedy_batch(h, pp, fp, 1, 1, 0, 0, None) == -1
    assert dll.ctcdec_greedy_batch(h, pp, fp, 1, 7, 0, 0, C.byref(res)) == -1   # dtype
    assert dll.ctcdec_greedy_batch(h, pp, fp, 1, 1, 0, 1, C.byref(res)) == -1   # fold
    assert dll.ctcdec_greedy_batch(h, pp, fp, -1, 1, 0, 0, C.byref(res)) == -1
    neg = np.ascontiguousarray([-1], dtype=np.int32)
    assert dll.ctcdec_greedy_batch(h, pp, neg.ctypes.data_as(C.POINTER(C.c_int32)), 1, 1, 0, 0, C.byref(res)) == -1
    null = np.zeros(1, dtype=np.uint64)
    assert dll.ctcdec_greedy_batch(h, null.ctypes.data_as(C.POINTER(C.c_void_p)), fp, 1, 1, 0, 0, C.byref(res)) == -1
    assert res.value is None
    ms, off = (C.c_double * 4)(), C.POINTER(C.c_int64)()
    assert dll.ctcdec_greedy_timing(None, ms, None, None) == -1
    assert dll.ctcdec_greedy_texts(None, None, C.byref(off), None) == -1
    assert dll.ctcdec_greedy_batch(h, pp, fp, 1, 1, 0, 0, C.byref(res)) == 0 and res.value
    dll.ctcdec_greedy_free(res)
    assert isinstance(B.EXPORTED_SYMBOLS, tuple) and "ctcdec_greedy_batch" in B.EXPORTED_SYMBOLS
