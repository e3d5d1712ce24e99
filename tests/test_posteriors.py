"""Frame posteriors (posteriors / posteriors_batch) on the CPU simulator of the kernel, which runs the body of ctc_posteriors
(csrc/ctc_align.h) itself with a one-thread context: every shape case of tests/align_util.py against the numpy
forward-backward of tests/posteriors_util.py, the single-path cases against align, tiny shapes against the posteriors by brute
force, the summaries without the dense table, batches and split launches equal to single calls float for float, a small call
on a workspace a large one left behind, and the refusals. The HIP build: tests/test_gpu_posteriors.py."""
import numpy as np
import pytest

from tests.posteriors_util import (GAMMA_TOL, check_posteriors, enumerate_np, same_bits, window_mask, yardstick)
from tests.score_util import SINGLE_PATH, case_input, neg_inf_case, normalisation_input, random_target, shape_cases
from tests.sim_util import sim_library  # noqa: F401
from tests.test_align import build, ragged_batch
from tests.token_logp_util import lp_matrix

SHAPES = shape_cases()
BY_NAME = {c[0]: c for c in SHAPES}
ENUMERATED = ((3, 4, [1]), (3, 5, [1, 1]), (4, 5, [1, 2]), (3, 6, [1, 2, 1]))


def table_bytes(x, target):
    return 32 * len(x) * ((2 * len(target) + 1 + 3) // 4)


@pytest.mark.parametrize("case", SHAPES, ids=[c[0] for c in SHAPES])
def test_shape_cases(case, sim_library):  # noqa: F811
    name, V, T, target, _dtype, _kind = case
    dec = build(V)
    x = case_input(case)
    blank = dec._alphabet.labels.index("")
    got = dec.posteriors(x, tokens=target)
    check_posteriors(got, yardstick(x, target, blank), T, target, name)
    assert got.logp == dec.score(x, tokens=[target])[0].logp
    assert dec.last_posteriors_launches == (1 if T > 0 else 0) and sum(dec.last_posteriors_launched) == (1 if T > 0 else 0)
    if T == 0:
        assert got.gamma.shape == (0, 1)
    if not target:
        assert (np.abs(got.gamma - 1.0) <= GAMMA_TOL).all()
    if name in SINGLE_PATH and T > 0:
        path = dec.align(x, tokens=target).path
        states, s = [], 0
        for t, c in enumerate(path.tolist()):  # the one alignment as states: a label moves to the next odd state
            if c == blank:
                s += s & 1
            elif not (s & 1 and t > 0 and path[t - 1] == c):
                s += 1 if not s & 1 else 2
            states.append(s)
        want = np.zeros_like(got.gamma)
        want[np.arange(T), states] = 1.0
        gap = float(np.abs(got.gamma - want).max())
        print("%s: against the indicator of align's path %.1e" % (name, gap))
        assert gap <= GAMMA_TOL, (name, gap)


@pytest.mark.parametrize("V,T,target", ENUMERATED, ids=["V%d_T%d_L%d" % (V, T, len(t)) for V, T, t in ENUMERATED])
def test_against_every_path(V, T, target, sim_library):  # noqa: F811
    dec = build(V)
    blank = dec._alphabet.labels.index("")
    assert blank not in target
    x = normalisation_input(V, T)
    got = dec.posteriors(x, tokens=target)
    logp, gamma = enumerate_np(lp_matrix(x), target, blank)
    gap = float(np.abs(got.gamma - gamma).max())
    print("V=%d T=%d %s: gamma against every path %.1e, logp %+.1e" % (V, T, target, gap, got.logp - logp))
    assert gap <= GAMMA_TOL and abs(got.logp - logp) <= 1e-9
    check_posteriors(got, yardstick(x, target, blank), T, target, "enumerated")


def test_neg_inf_logits(sim_library):  # noqa: F811
    dec = build(29)
    x, target = neg_inf_case()
    got = dec.posteriors(x, tokens=target)
    assert np.isfinite(got.logp) and np.isfinite(got.logp_backward)
    check_posteriors(got, yardstick(x, target, dec._alphabet.labels.index("")), len(x), target, "-inf logits")


def test_summaries_without_the_table(sim_library):  # noqa: F811
    for name in ("L129_T300", "V130_f16", "V29_probs", "empty_target", "T0"):
        case = BY_NAME[name]
        dec = build(case[1])
        x = case_input(case)
        dense, lean = dec.posteriors(x, tokens=case[3]), dec.posteriors(x, tokens=case[3], dense=False)
        assert lean.gamma is None and lean.token_post is None and lean.blank_post is None
        assert same_bits(dense, lean, dense=False), name


def test_batch_equals_single_calls_and_split_launches(sim_library):  # noqa: F811
    dec = build(29)
    blank = dec._alphabet.labels.index("")
    xs, targets = ragged_batch()
    batch = dec.posteriors_batch(xs, tokens=targets)
    assert dec.last_posteriors_launches == 1 and dec.last_posteriors_launched == (sum(1 for x in xs if len(x)), 0)
    singles = [dec.posteriors(x, tokens=t) for x, t in zip(xs, targets)]
    for u, (x, t) in enumerate(zip(xs, targets)):
        assert same_bits(batch[u], singles[u]), u
        check_posteriors(batch[u], yardstick(x, t, blank), len(x), t, "utt %d" % u)
    # padded into one [B, T, V] array: every row of an utterance is a frame
    T = max(len(x) for x in xs)
    pad = np.zeros((len(xs), T, 29))
    for u, x in enumerate(xs):
        pad[u, : len(x)] = x
    cube = dec.posteriors_batch(pad, tokens=targets)
    for u, t in enumerate(targets):
        assert same_bits(cube[u], dec.posteriors(pad[u], tokens=t)), u
    # a budget a third of the batch's tables: three launches or more, the same floats
    sizes = [table_bytes(x, t) for x, t in zip(xs, targets)]
    budget = max(max(sizes), sum(sizes) // 3)
    split = dec.posteriors_batch(xs, tokens=targets, _table_budget=budget)
    assert dec.last_posteriors_launches >= 3, dec.last_posteriors_launches
    assert all(same_bits(a, b) for a, b in zip(split, batch))
    lean = dec.posteriors_batch(xs, tokens=targets, dense=False, _table_budget=budget)
    assert all(b.gamma is None and same_bits(a, b, dense=False) for a, b in zip(batch, lean))
    big = int(np.argmax(sizes))
    with pytest.raises(ValueError, match="utterance %d .*table" % big):
        dec.posteriors_batch(xs, tokens=targets, _table_budget=max(sizes) - 1)


def test_small_call_on_a_stale_workspace(sim_library):  # noqa: F811
    """The tables come from a grow-only workspace: after a large call a small one finds the large one's posteriors in it,
    and must neither read them nor leave them in what it returns."""
    large = BY_NAME["L129_T300"]
    dec = build(29)
    got = dec.posteriors(case_input(large), tokens=large[3])
    assert got.gamma.shape == (300, 259) and float(got.gamma.max()) > 0.5
    for name in ("T_eq_L_no_blanks", "aaa_at_bound"):
        case = BY_NAME[name]
        x = case_input(case)
        if case[1] != 29:  # (aaa_at_bound has five labels: the same floats under the first five of 29)
            x = np.concatenate([x, np.full((len(x), 29 - case[1]), -40.0)], axis=1)
        stale, fresh = dec.posteriors(x, tokens=case[3]), build(29).posteriors(x, tokens=case[3])
        assert same_bits(stale, fresh), name
        assert (stale.gamma[~window_mask(*stale.gamma.shape)] == 0.0).all(), name
        check_posteriors(stale, yardstick(x, case[3], 0), len(x), case[3], name + " after a large call")


def test_bad_arguments(sim_library):  # noqa: F811
    from pyctcdecode_amd import build_ctcdecoder

    dec = build(5)
    labels = dec._alphabet.labels
    x = np.zeros((9, 5))
    with pytest.raises(ValueError, match=r"no alignment for utterances \[1\]"):
        dec.posteriors_batch([x, x[:2]], tokens=[[2, 3], [2, 2]])
    got = dec.posteriors_batch([x, x[:2], x], tokens=[[2, 3], [2, 2], [3]], strict=False)
    assert got[1] is None and got[0].tokens == [2, 3] and got[2].gamma.shape == (9, 3)
    assert dec.posteriors_batch([x[:1]], tokens=[[2, 3]], strict=False) == [None]
    with pytest.raises(ValueError, match="utterance 0 .*limit of 2047"):
        dec.posteriors(np.zeros((2100, 5)), tokens=random_target(np.random.default_rng(1), 2048, 5))
    for bad in ([labels.index("")], [5], [-1], [2.0], [True]):
        with pytest.raises(ValueError, match=r"tokens\[1\].*label id"):
            dec.posteriors_batch([x, x], tokens=[[2], bad])
    with pytest.raises(ValueError, match="targets for 2 utterances"):
        dec.posteriors_batch([x, x], "ab")
    with pytest.raises(ValueError, match="'z'"):
        dec.posteriors(x, "ab z")
    with pytest.raises(ValueError, match="exactly one"):
        dec.posteriors(x, "ab", tokens=[2, 3])
    with pytest.raises(ValueError, match="exactly one"):
        dec.posteriors_batch([x])
    with pytest.raises(ValueError):
        dec.posteriors(np.zeros((9, 6)), "ab")
    assert dec.posteriors_batch([], []) == []
    text = dec.posteriors(x, "  ab  a ")
    assert text.text == "ab a" and text.tokens == [labels.index(c) for c in "ab a"]
    assert same_bits(text, dec.posteriors(x, tokens=text.tokens))
    bpe = build_ctcdecoder(["<unk>", "▁bug", "s", "▁bun", "ny", "▁", "n", "▁a"])
    with pytest.raises(ValueError, match="tokens="):
        bpe.posteriors(np.zeros((25, len(bpe._alphabet.labels))), "bugs bunny")


def test_native_call_validates_what_it_indexes_with(sim_library):  # noqa: F811
    """The C entry point on its own: null pointers, offsets that do not start at 0 or decrease, a label outside the alphabet,
    the blank, too few frames, too many labels and a table above the budget are error codes before anything is launched."""
    import ctypes as C

    dec = build(5)
    blank = dec._alphabet.labels.index("")
    x = np.zeros((4, 5))
    dll = dec._lib.dll

    def call(target, off=None, frames=4, null=(), budget=0):
        ptrs = (C.c_void_p * 1)(None if "x" in null else x.ctypes.data)
        fr = (C.c_int32 * 1)(frames)
        flat = np.array(list(target) or [0], dtype=np.int32)
        lo = np.array(off if off is not None else [0, len(target)], dtype=np.int64)
        res = C.c_void_p()
        rc = dll.ctcdec_posteriors_batch(
            None if "dec" in null else dec._handle, None if "ptrs" in null else ptrs, None if "frames" in null else fr, 1, 1, 0,
            None if "off" in null else lo.ctypes.data_as(C.POINTER(C.c_int64)),
            None if "labels" in null else flat.ctypes.data_as(C.POINTER(C.c_int32)), 1, budget,
            None if "out" in null else C.byref(res))
        if rc == 0:
            dll.ctcdec_posteriors_free(res)
        return rc

    assert call([2, 3]) == 0
    for what in ("dec", "ptrs", "frames", "off", "labels", "out", "x"):
        assert call([2, 3], null=(what,)) == -1, what
    assert call([2, 5]) == -1 and call([-1]) == -1 and call([blank]) == -1
    assert call([2, 3], off=[1, 2]) == -1 and call([2, 3], off=[0, -1]) == -1
    assert call([2, 3], frames=-1) == -1 and call([2, 2, 2], frames=4) == -1 and call([2, 3], budget=-1) == -1
    assert call([2] * 2048, frames=4) == -4
    assert call([2, 3], budget=255) == -4 and call([2, 3], budget=256) == 0
    assert call([2, 3]) == 0  # (the decoder still works)


def test_parallel_refuses(sim_library):  # noqa: F811
    from pyctcdecode_amd.parallel import DevicePool, posteriors_batch_sharded

    dec = build(5)
    with pytest.raises(NotImplementedError):
        posteriors_batch_sharded(dec, [np.zeros((3, 5))], ["a"])
    with DevicePool(dec, devices=[0], library=sim_library.path) as pool:
        with pytest.raises(NotImplementedError):
            pool.posteriors_batch([np.zeros((3, 5))], ["a"])
        with pytest.raises(NotImplementedError):
            pool.posteriors(np.zeros((3, 5)), "a")
