"""Transcript gradient (gradient / gradient_batch) on the CPU simulator, which runs the body of ctc_grad_rows
(csrc/ctc_align.h) itself with a one-thread context behind a dense ctc_posteriors pass: the yardsticks of tests/grad_util.py
against each other first, then every shape case against the numpy one, the clipped cases, the row properties, batches and split
launches equal to single calls float for float, a repeated call, a small call on a workspace a large one left behind, and the
refusals. The HIP build and ctc_loss: tests/test_gpu_gradient.py."""
import numpy as np
import pytest

from tests.grad_util import (SCORE_TOL, YARDSTICK_TOL, RECURSION_MAX_T, check_gradient, check_rows, clipped_target_case,
                             grad_np, grad_recursion, grad_torch, looks_like_probs, neg_inf_case, same_bits, unclipped)
from tests.score_util import case_input, random_logits, random_target, shape_cases
from tests.sim_util import sim_library  # noqa: F401
from tests.test_align import build, ragged_batch
from tests.test_posteriors import table_bytes

SHAPES = shape_cases()
BY_NAME = {c[0]: c for c in SHAPES}
# (name, V, x, target, entries at the floor): every shape case with frames, and the two cases that clip
CASES = [(c[0], c[1], case_input(c), c[3], 0) for c in SHAPES if c[2] > 0]
CASES.append(("neg_inf",) + (29,) + neg_inf_case() + (10,))
CASES.append(("clipped_target",) + (12,) + clipped_target_case() + (31,))


@pytest.fixture(scope="module")
def references():
    """Yardstick 1 of every case, computed once."""
    return {name: grad_np(x, target, 0) for name, _V, x, target, _n in CASES}


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_yardsticks_agree(case, references):
    """Before anything of ours is asked: numpy against torch's ctc_loss (logits, nothing clipped) and against autograd through
    the hand-written recursion (probabilities, clipped entries, and every case short enough for it)."""
    name, _V, x, target, n_floor = case
    logp, grad = references[name]
    assert int((~unclipped(x)).sum()) == n_floor, name
    probs = looks_like_probs(x)
    assert probs == (name == "V29_probs")
    others = []
    if not probs and n_floor == 0:
        others.append(("torch ctc_loss",) + grad_torch(x, target, 0))
    if len(x) <= RECURSION_MAX_T:
        others.append(("recursion",) + grad_recursion(x, target, 0))
    assert others and (len(others) == 2 or len(x) > RECURSION_MAX_T or probs or n_floor), name
    scale = x.astype(np.float64) if probs else 1.0  # (G / p is unbounded: a probability-like utterance is compared as p * grad)
    for who, other_logp, other_grad in others:
        gap = float(np.abs(scale * (grad - other_grad)).max())
        print("%s: numpy against %s: grad %.1e, logp %.1e" % (name, who, gap, abs(logp - other_logp)))
        assert gap <= YARDSTICK_TOL and abs(logp - other_logp) <= YARDSTICK_TOL, (name, who, gap)


@pytest.mark.parametrize("case", SHAPES, ids=[c[0] for c in SHAPES])
def test_shape_cases(case, sim_library, references):  # noqa: F811
    name, V, T, target, _dtype, kind = case
    dec = build(V)
    x = case_input(case)
    got = dec.gradient(x, tokens=target)
    want = references[name] if T > 0 else (0.0, np.zeros((0, V)))
    grad = check_gradient(got, want, x, target, name)
    assert got.logp == dec.score(x, tokens=[target])[0].logp
    # one ctc_posteriors launch and one ctc_grad_rows launch; nothing without frames
    assert dec.last_gradient_launches == (2 if T > 0 else 0) and sum(dec.last_gradient_launched) == (1 if T > 0 else 0)
    assert len(dec.last_gradient_timing_ms) == 5
    if T > 0 and kind != "probs":
        check_rows(grad, x, target, 0, name)
    assert same_bits(got, dec.gradient(x, tokens=target))  # (a repeated call on the same decoder)


@pytest.mark.parametrize("which", ["neg_inf", "clipped_target"])
def test_clipped_entries(which, sim_library, references):  # noqa: F811
    _name, V, x, target, n_floor = [c for c in CASES if c[0] == which][0]
    dec = build(V)
    got = dec.gradient(x, tokens=target)
    grad = check_gradient(got, references[which], x, target, which)
    assert got.logp == dec.score(x, tokens=[target])[0].logp and np.isfinite(grad).all()
    # a clipped entry keeps no share of gamma: its gradient is -softmax * M alone, so not positive -- target label or not
    floor = ~unclipped(x)
    assert int(floor.sum()) == n_floor and (grad[floor] <= 0.0).all()
    assert floor[:, target].any()  # (the case does clip target entries)


def test_batch_equals_single_calls_and_split_launches(sim_library):  # noqa: F811
    dec = build(29)
    xs, targets = ragged_batch()
    batch = dec.gradient_batch(xs, tokens=targets)
    assert dec.last_gradient_launches == 2 and dec.last_gradient_launched == (sum(1 for x in xs if len(x)), 0)
    for u, (x, t) in enumerate(zip(xs, targets)):
        assert same_bits(batch[u], dec.gradient(x, tokens=t)), u
        check_gradient(batch[u], grad_np(x, t, 0) if len(x) else (0.0, np.zeros((0, 29))), x, t, "utt %d" % u)
    # padded into one [B, T, V] array: every row of an utterance is a frame
    T = max(len(x) for x in xs)
    pad = np.zeros((len(xs), T, 29))
    for u, x in enumerate(xs):
        pad[u, : len(x)] = x
    cube = dec.gradient_batch(pad, tokens=targets)
    for u, t in enumerate(targets):
        assert same_bits(cube[u], dec.gradient(pad[u], tokens=t)), u
    # a budget a third of the batch's tables: three launches of each kernel or more, the same floats
    sizes = [table_bytes(x, t) for x, t in zip(xs, targets)]
    split = dec.gradient_batch(xs, tokens=targets, _table_budget=max(max(sizes), sum(sizes) // 3))
    assert dec.last_gradient_launches >= 6, dec.last_gradient_launches
    assert all(same_bits(a, b) for a, b in zip(split, batch))
    big = int(np.argmax(sizes))
    with pytest.raises(ValueError, match="utterance %d .*table" % big):
        dec.gradient_batch(xs, tokens=targets, _table_budget=max(sizes) - 1)
    # both ctc_posteriors instantiations in one call
    rng = np.random.default_rng(3)
    x = random_logits(rng, 700, 29)
    mixed = [random_target(rng, L, 29, doubled=min(2, L // 2)) for L in (3, 511, 512, 40)]
    got = dec.gradient_batch([x] * 4, tokens=mixed)
    assert dec.last_gradient_launched == (3, 1) and dec.last_gradient_launches == 3
    for t, g in zip(mixed, got):
        assert same_bits(g, dec.gradient(x, tokens=t)), len(t)
        assert g.logp == dec.score(x, tokens=[t])[0].logp


def test_small_call_on_a_stale_workspace(sim_library):  # noqa: F811
    """The tables and the gradient rows come from grow-only workspaces: after a large call a small one finds the large one's
    data in them, and must neither read it nor leave it in what it returns."""
    large = BY_NAME["L129_T300"]
    dec = build(29)
    got = dec.gradient(case_input(large), tokens=large[3])
    assert got.grad.shape == (300, 29) and float(np.abs(got.grad).max()) > 0.5
    for name in ("T_eq_L_no_blanks", "aaa_at_bound"):
        case = BY_NAME[name]
        x = case_input(case)
        if case[1] != 29:  # (aaa_at_bound has five labels: the same floats under the first five of 29)
            x = np.concatenate([x, np.full((len(x), 29 - case[1]), -40.0)], axis=1)
        stale, fresh = dec.gradient(x, tokens=case[3]), build(29).gradient(x, tokens=case[3])
        assert same_bits(stale, fresh), name
        check_gradient(stale, grad_np(x, case[3], 0), x, case[3], name + " after a large call")


def test_bad_arguments(sim_library):  # noqa: F811
    from pyctcdecode_amd import TranscriptGradient, build_ctcdecoder

    dec = build(5)
    labels = dec._alphabet.labels
    x = np.zeros((9, 5))
    with pytest.raises(ValueError, match=r"no alignment for utterances \[1\]"):
        dec.gradient_batch([x, x[:2]], tokens=[[2, 3], [2, 2]])
    got = dec.gradient_batch([x, x[:2], x], tokens=[[2, 3], [2, 2], [3]], strict=False)
    assert got[1] is None and got[0].tokens == [2, 3] and got[2].grad.shape == (9, 5) and isinstance(got[0], TranscriptGradient)
    assert dec.gradient_batch([x[:1]], tokens=[[2, 3]], strict=False) == [None]
    with pytest.raises(ValueError, match="utterance 0 .*limit of 2047"):
        dec.gradient(np.zeros((2100, 5)), tokens=random_target(np.random.default_rng(1), 2048, 5))
    for bad in ([labels.index("")], [5], [-1], [2.0], [True]):
        with pytest.raises(ValueError, match=r"tokens\[1\].*label id"):
            dec.gradient_batch([x, x], tokens=[[2], bad])
    with pytest.raises(ValueError, match="targets for 2 utterances"):
        dec.gradient_batch([x, x], "ab")
    with pytest.raises(ValueError, match="exactly one"):
        dec.gradient(x, "ab", tokens=[2, 3])
    with pytest.raises(ValueError):
        dec.gradient(np.zeros((9, 6)), "ab")
    assert dec.gradient_batch([], []) == []
    text = dec.gradient(x, "  ab  a ")
    assert text.text == "ab a" and text.tokens == [labels.index(c) for c in "ab a"]
    assert same_bits(text, dec.gradient(x, tokens=text.tokens))
    bpe = build_ctcdecoder(["<unk>", "▁bug", "s", "▁bun", "ny", "▁", "n", "▁a"])
    with pytest.raises(ValueError, match="tokens="):
        bpe.gradient(np.zeros((25, len(bpe._alphabet.labels))), "bugs bunny")


def test_native_call_validates_what_it_indexes_with(sim_library):  # noqa: F811
    """The C entry point on its own: null pointers, a label outside the alphabet, the blank, too few frames, too many labels, a
    table above the budget and a gradient type that does not go with the logits are error codes before anything is launched."""
    import ctypes as C

    dec = build(5)
    blank = dec._alphabet.labels.index("")
    x = np.zeros((4, 5))
    grad = np.full((4, 5), 7.0)
    dll = dec._lib.dll

    def call(target, frames=4, null=(), budget=0, grad_dtype=1):
        ptrs = (C.c_void_p * 1)(None if "x" in null else x.ctypes.data)
        outs = (C.c_void_p * 1)(None if "grad" in null else grad.ctypes.data)
        fr = (C.c_int32 * 1)(frames)
        flat = np.array(list(target) or [0], dtype=np.int32)
        lo = np.array([0, len(target)], dtype=np.int64)
        logp = (C.c_double * 1)()
        return dll.ctcdec_gradient_batch(
            None if "dec" in null else dec._handle, None if "ptrs" in null else ptrs, None if "frames" in null else fr, 1, 1, 0,
            None if "off" in null else lo.ctypes.data_as(C.POINTER(C.c_int64)),
            None if "labels" in null else flat.ctypes.data_as(C.POINTER(C.c_int32)), None if "outs" in null else outs, grad_dtype,
            budget, None if "logp" in null else logp, None, None, None)

    assert call([2, 3]) == 0 and abs(float(grad.sum())) < 1e-9 and not (grad == 7.0).any()
    for what in ("dec", "ptrs", "frames", "off", "labels", "outs", "logp", "x", "grad"):
        assert call([2, 3], null=(what,)) == -1, what
    assert call([2, 5]) == -1 and call([-1]) == -1 and call([blank]) == -1
    assert call([2, 3], frames=-1) == -1 and call([2, 2, 2], frames=4) == -1 and call([2, 3], budget=-1) == -1
    assert call([2, 3], grad_dtype=0) == -1
    assert call([2] * 2048, frames=4) == -4
    assert call([2, 3], budget=255) == -4 and call([2, 3], budget=256) == 0


def test_parallel_refuses(sim_library):  # noqa: F811
    from pyctcdecode_amd.parallel import DevicePool, gradient_batch_sharded

    dec = build(5)
    with pytest.raises(NotImplementedError):
        gradient_batch_sharded(dec, [np.zeros((3, 5))], ["a"])
    with DevicePool(dec, devices=[0], library=sim_library.path) as pool:
        with pytest.raises(NotImplementedError):
            pool.gradient_batch([np.zeros((3, 5))], ["a"])
        with pytest.raises(NotImplementedError):
            pool.gradient(np.zeros((3, 5)), "a")
