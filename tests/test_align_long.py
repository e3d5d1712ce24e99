"""Forced alignment of long transcripts (align_long / align_long_batch) on the CPU simulator of the kernels, which runs the
body of ctc_viterbi_long (csrc/ctc_align.h) itself with a one-thread context: every shape case of tests/align_util.py equal to
align bit for bit at every forced segment length, targets above align's 2047 labels against the numpy Viterbi, mixed batches,
budgets, and the refusals in Python and through the C entry point. The HIP build: tests/test_gpu_align_long.py."""
import ctypes as C

import numpy as np
import pytest

from tests.align_long_util import (ABOVE, LONG_MAX_LABELS, SHAPES, build, case_input, check_above, check_equals_align, crosses,
                                   mixed_batch, plan_of, same)
from tests.align_util import SCORE_TOL, check_aligned, random_logits, random_target
from tests.sim_util import sim_library  # noqa: F401


@pytest.mark.parametrize("case", SHAPES, ids=[c[0] for c in SHAPES])
def test_equals_align_at_every_segment_length(case, sim_library):  # noqa: F811
    name, V, T, target, _dtype, _kind = case
    dec = build(V)
    x = case_input(case)
    at7 = check_equals_align(dec, x, target, name, T)
    if name.endswith("_T300"):
        # a label's span that lies on both sides of a segment boundary: align on this tree finds one in these inputs, and the
        # result cut at 7 frames holds it
        assert crosses(dec.align(x, tokens=target), 7), name
        assert crosses(at7, 7), name


def test_plan_is_a_function_of_frames_labels_budget_and_segment(sim_library):  # noqa: F811
    dec = build(5)
    plan = dec._align_long_plan
    assert plan(0, 0, 1 << 30, 0) == (0, 0, 0) and plan(1, 1, 1 << 30, 0) == (1, 0, 1 + 64)
    assert plan(300, 127, 1 << 30, 0) == (300, 1, 300 * 64 + 64 * 64)  # the whole table fits: one segment, no checkpoints
    assert plan(300, 127, 1 << 30, 7) == (7, 43, 7 * 64 + 32 * 64 * 43 + 64 * 64)
    assert plan(300, 127, 1 << 30, 305) == plan(300, 127, 1 << 30, 300)
    assert plan(300, 127, 300 * 64 + 64 * 64 - 1, 0) == (98, 4, 98 * 64 + 32 * 64 * 4 + 64 * 64)  # ceil(sqrt(32 * 300)) = 98
    # the hour of the issue: 180000 frames, 40000 labels -- about 100 MB where the whole table is 3.6 GB
    K, n, b = plan(180000, 40000, 1 << 30, 0)
    assert (K, n) == (2400, 75) and b == 2400 * 20001 + 32 * 20001 * 75 + 64 * 20001 and b < 100 * 2 ** 20
    # the native call reports what the Python rule plans
    rng = np.random.default_rng(2)
    x, target = random_logits(rng, 300, 5), random_target(rng, 127, 5)
    whole = dec.align_long_batch([x], tokens=[target])[0]
    assert dec.last_align_long_plan == [(300, 1)]
    cut = dec.align_long_batch([x], tokens=[target], _bp_budget=300 * 64 + 64 * 64 - 1)[0]
    assert dec.last_align_long_plan == [(98, 4)] and same(whole, cut)


@pytest.mark.parametrize("case", ABOVE, ids=[c[0] for c in ABOVE])
def test_above_2047_labels_against_numpy(case, sim_library):  # noqa: F811
    """Largest |score - numpy optimum| seen: 0 in all four cases, under the float64 SCORE_TOL = 1e-9 ("Forced
    alignment of long transcripts")."""
    assert check_above(build(case[1]), case) <= SCORE_TOL


def test_mixed_batch_equals_single_calls(sim_library):  # noqa: F811
    dec = build(29)
    xs, targets, bad = mixed_batch()
    with pytest.raises(ValueError, match=r"\[%d\]" % bad):
        dec.align_long_batch(xs, tokens=targets)
    for K in (0, 7):
        batch = dec.align_long_batch(xs, tokens=targets, confidence="mean", strict=False, _segment_frames=K)
        assert dec.last_align_long_plan == [plan_of(len(x), K) for u, x in enumerate(xs) if u != bad]
        assert dec.last_align_long_launches == 1
        assert batch[bad] is None
        for u, (x, target) in enumerate(zip(xs, targets)):
            if u == bad:
                with pytest.raises(ValueError, match="no path"):
                    dec.align_long(x, tokens=target)
                continue
            one = dec.align_long_batch([x], tokens=[target], confidence="mean", _segment_frames=K)[0]
            assert same(batch[u], one), (K, u)
            if len(target) <= 2047:
                assert same(batch[u], dec.align(x, tokens=target, confidence="mean")), (K, u)
            if len(x):
                check_aligned(batch[u], x, target, dec, "mean", "utt %d" % u)
    empty = batch[1]
    assert empty.text == "" and empty.path.shape == (0,) and empty.score == 0.0 and empty.token_frames == []


def test_small_budget_takes_several_launches(sim_library):  # noqa: F811
    dec = build(29)
    xs, targets, bad = mixed_batch()
    xs, targets = [x for u, x in enumerate(xs) if u != bad], [t for u, t in enumerate(targets) if u != bad]
    whole = dec.align_long_batch(xs, tokens=targets, confidence="max")
    assert dec.last_align_long_launches == 1 and all(n <= 1 for _k, n in dec.last_align_long_plan)
    # below the whole table of the largest utterance (2300 frames, 2049 labels): that one is cut, and the batch no longer fits one launch
    budget = 640000  # (its plan in segments takes 639600 bytes)
    assert dec._align_long_plan(2300, 2049, budget, 0)[:2] == (272, 9)
    split = dec.align_long_batch(xs, tokens=targets, confidence="max", _bp_budget=budget)
    assert dec.last_align_long_launches > 1
    assert dec.last_align_long_plan[3] == (272, 9)
    assert all(same(a, b) for a, b in zip(whole, split))
    # below that utterance's smallest plan: refused by name, with the bytes
    smallest = dec._align_long_plan(2300, 2049, 1, 0)[2]
    with pytest.raises(ValueError, match=r"utterance 3 .* %d bytes" % smallest):
        dec.align_long_batch(xs, tokens=targets, _bp_budget=smallest - 1)
    assert all(same(a, b) for a, b in zip(whole, dec.align_long_batch(xs, tokens=targets, confidence="max")))


def test_bad_arguments(sim_library):  # noqa: F811
    from pyctcdecode_amd import build_ctcdecoder
    from pyctcdecode_amd.decoder import _DeviceStreams, _ResidentBeams

    dec = build(5)
    labels = dec._alphabet.labels
    x = np.zeros((9, 5))
    good = dec.align(x, tokens=[2, 3])

    def still_aligns():
        assert same(dec.align_long(x, tokens=[2, 3]), good)

    # the cap, by the check alone: nothing is staged for a target this long
    with pytest.raises(ValueError, match="limit of %d" % LONG_MAX_LABELS):
        dec._one_target_each("align_long", [x], None, [np.full(LONG_MAX_LABELS + 1, 2)], LONG_MAX_LABELS)
    dec._one_target_each("align_long", [x], None, [[2] * 2048], LONG_MAX_LABELS)  # (above align's limit: accepted)
    still_aligns()
    for bad in ([labels.index("")], [5], [-1], [2.0], [True]):
        with pytest.raises(ValueError, match="label id"):
            dec.align_long(x, tokens=bad)
    still_aligns()
    for bad in (-1, 1.5, True, 2 ** 31):
        with pytest.raises(ValueError, match="_segment_frames"):
            dec.align_long_batch([x], tokens=[[2, 3]], _segment_frames=bad)
    still_aligns()
    with pytest.raises(ValueError, match="exactly one"):
        dec.align_long(x, "ab", tokens=[2, 3])
    with pytest.raises(ValueError, match="2 targets for 1"):
        dec.align_long_batch([x], ["a", "b"])
    with pytest.raises(ValueError):
        dec.align_long(x, "ab", confidence="median")
    assert dec.align_long_batch([], []) == []
    still_aligns()
    # a text under a BPE alphabet
    bpe = build_ctcdecoder(["<unk>", "▁bug", "s", "▁bun", "ny"])
    with pytest.raises(ValueError, match="tokens="):
        bpe.align_long(np.zeros((9, len(bpe._alphabet.labels))), "bugs bunny")
    # streams: the frames they have consumed are not kept
    for stream in (object.__new__(_DeviceStreams), list.__new__(_ResidentBeams)):
        with pytest.raises(NotImplementedError):
            dec.align_long(stream, tokens=[2, 3])
        with pytest.raises(NotImplementedError):
            dec.align_long_batch([stream], tokens=[[2, 3]])
        with pytest.raises(NotImplementedError):
            dec.align_long_batch(stream, tokens=[[2, 3]])
    still_aligns()


def test_native_call_validates_what_it_indexes_with(sim_library):  # noqa: F811
    """The C entry point on its own: error codes before anything is launched, and the plan of both kinds of alignment."""
    dec = build(5)
    blank = dec._alphabet.labels.index("")
    x = np.zeros((4, 5))
    dll = dec._lib.dll
    i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)

    def call(target, frames=4, off=None, segment=0, budget=0, out=True, long=True):
        ptrs = (C.c_void_p * 1)(x.ctypes.data)
        fr = (C.c_int32 * 1)(frames)
        t = np.array(target or [0], dtype=np.int32)
        o = np.array(off or [0, len(target)], dtype=np.int64)
        res = C.c_void_p()
        head = (dec._handle, ptrs, fr, 1, 1, 0, t.ctypes.data_as(i32p), o.ctypes.data_as(i64p), 0, budget)
        if long:
            rc = dll.ctcdec_align_long_batch(*head, segment, C.byref(res) if out else None)
        else:
            rc = dll.ctcdec_align_batch(*head, C.byref(res))
        plan = None
        if rc == 0:
            sf, ns, n = i32p(), i32p(), C.c_int64()
            assert dll.ctcdec_alignment_plan(res, C.byref(sf), C.byref(ns), C.byref(n)) == 0 and n.value == 1
            plan = (sf[0], ns[0])
            assert dll.ctcdec_alignment_plan(res, None, C.byref(ns), C.byref(n)) == -1
            dll.ctcdec_alignment_free(res)
        return rc, plan

    assert call([2, 3]) == (0, (4, 1)) and call([2, 3], segment=2) == (0, (2, 2)) and call([2, 3], segment=9) == (0, (4, 1))
    assert call([2, 3], long=False) == (0, (4, 1))  # ctcdec_align_batch: one segment of all frames
    assert call([2, 3], frames=1, off=[0, 0]) == (0, (1, 0)) and call([], frames=0) == (0, (0, 0))
    assert call([2, 5])[0] == -1 and call([-1])[0] == -1 and call([blank])[0] == -1
    assert call([2, 2, 2])[0] == -1  # (needs five frames)
    assert call([2, 3], off=[0, -1])[0] == -1 and call([2, 3], off=[1, 2])[0] == -1
    assert call([2, 3], frames=-1)[0] == -1
    assert call([2, 3], segment=-1)[0] == -1
    assert call([2, 3], out=False)[0] == -1
    assert call([2, 3], budget=-1)[0] == -1
    # more labels than the cap: the offsets alone say so (the labels are never read)
    assert call([2], off=[0, LONG_MAX_LABELS + 1])[0] == -4
    assert b"utterance 0" in dll.ctcdec_last_error() and str(LONG_MAX_LABELS).encode() in dll.ctcdec_last_error()
    # a budget below the smallest plan: 4 frames, 2 labels, nch = 2 -- K = 4 gives 8 + 128 bytes
    assert call([2, 3], budget=136)[0] == 0 and call([2, 3], budget=135)[0] == -4
    assert b"utterance 0" in dll.ctcdec_last_error() and b"136 bytes" in dll.ctcdec_last_error()
    assert call([2, 3]) == (0, (4, 1))


def test_parallel_refuses(sim_library):  # noqa: F811
    from pyctcdecode_amd.parallel import DevicePool, align_long_batch_sharded

    dec = build(5)
    with pytest.raises(NotImplementedError):
        align_long_batch_sharded(dec, [np.zeros((3, 5))], ["a"])
    with DevicePool(dec, devices=[0], library=sim_library.path) as pool:
        with pytest.raises(NotImplementedError):
            pool.align_long_batch([np.zeros((3, 5))], ["a"])
        with pytest.raises(NotImplementedError):
            pool.align_long([np.zeros((3, 5))], ["a"])
    assert dec.align_long(np.zeros((3, 5)), "a").text == "a"
