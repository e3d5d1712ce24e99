"""Transcript likelihood of long transcripts (score_long / score_long_batch) on the CPU simulator of the kernels, which runs the
body of ctc_forward_tile (csrc/ctc_align.h) itself, tile by tile in launch order, with a one-thread context: every shape case
of tests/align_util.py equal to score bit for bit at every tile shape, hypotheses above score's 2047 labels against the numpy
recursion, several hypotheses per utterance, budgets, and the refusals in Python and through the C entry point. The HIP build:
tests/test_gpu_score_long.py."""
import ctypes as C

import numpy as np
import pytest

from tests.score_long_util import (ABOVE, LONG_MAX_LABELS, SHAPES, build, case_input, check_above, check_equals_score,
                                   check_hypotheses_batch, hypotheses_batch)
from tests.sim_util import sim_library  # noqa: F401


@pytest.mark.parametrize("case", SHAPES, ids=[c[0] for c in SHAPES])
def test_equals_score_at_every_tile_shape(case, sim_library):  # noqa: F811
    name, V, T, target, _dtype, _kind = case
    skipped = check_equals_score(build(V), case_input(case), target, name, T)
    if name.endswith("_T300"):  # 300 frames by 16 to 65 groups: most of the triangles outside the window are never launched
        assert skipped, name


def test_plan_is_a_function_of_frames_labels_budget_and_tile(sim_library):  # noqa: F811
    plan = build(5)._score_long_plan
    assert plan(0, 0, 1 << 30, 0, 0) == (0, 0, 0, 0, 0) and plan(1, 1, 1 << 30, 0, 0) == (256, 1, 1, 1, 32)
    assert plan(300, 127, 1 << 30, 0, 0) == (256, 300, 1, 1, 32 * 64)      # one state block: one tile of all frames
    assert plan(300, 127, 1 << 30, 3, 7) == (3, 7, 22, 43, 32 * 64 + 24 * 21 * 7)
    assert plan(300, 127, 1 << 30, 3, 305) == plan(300, 127, 1 << 30, 3, 300)
    assert plan(2100, 2048, 1 << 30, 0, 0) == (256, 64, 5, 33, 32 * 1025 + 24 * 4 * 64)
    assert plan(2100, 2048, 32 * 1025 + 24 * 4 * 64 - 1, 0, 0) == (256, 63, 5, 34, 32 * 1025 + 24 * 4 * 63)  # the budget shortens FB
    assert plan(2100, 2048, 1, 0, 0) == (256, 1, 5, 2100, 32 * 1025 + 24 * 4)
    # the hour of DESIGN.md: 180000 frames, 40000 labels -- 79 state blocks, 2813 time blocks, 760 KB
    assert plan(180000, 40000, 1 << 30, 0, 0) == (256, 64, 79, 2813, 32 * 20001 + 24 * 78 * 64)


@pytest.mark.parametrize("case", ABOVE, ids=[c[0] for c in ABOVE])
def test_above_2047_labels_against_numpy(case, sim_library):  # noqa: F811
    """Largest |logp - numpy| seen on the simulator: 7.3e-12 (L4100_T4400: logp -10890.5, bound 8.5e-8; V29_L3000_T9000_f32:
    logp -33989.7, bound 5.4e-7); 0 at L2048_T2100. The asserted bound is 8 T eps |logp| (tests/score_long_util.check_above)."""
    check_above(build(case[1]), case)


@pytest.mark.parametrize("dtype", [np.float16, np.float32, np.float64])
def test_hypotheses_batch_equals_single_calls(dtype, sim_library):  # noqa: F811
    xs, hyps, dead = hypotheses_batch(dtype)
    batch = check_hypotheses_batch(build(29), xs, hyps, dead)
    assert batch[0][3].text == "" and np.isfinite(batch[0][3].logp) and batch[1][1].tokens == []


def test_budget_and_refusals(sim_library):  # noqa: F811
    from pyctcdecode_amd.decoder import _DeviceStreams, _ResidentBeams
    from pyctcdecode_amd.parallel import DevicePool, score_long_batch_sharded

    dec = build(29)
    xs, hyps, _dead = hypotheses_batch()
    whole = dec.score_long_batch(xs, tokens=hyps)
    smallest = dec._score_long_plan(2500, 2100, 1, 0, 0)[4]
    split = dec.score_long_batch(xs, tokens=hyps, _budget=smallest)  # the largest hypothesis alone fills a launch group
    assert dec.last_score_long_groups > 1 and dec.last_score_long_plan[0] == dec._score_long_plan(2500, 2100, smallest, 0, 0)
    assert [[h.logp for h in cur] for cur in split] == [[h.logp for h in cur] for cur in whole]
    with pytest.raises(ValueError, match=r"utterance 0, hypothesis 0 .* %d bytes" % smallest):
        dec.score_long_batch(xs, tokens=hyps, _budget=smallest - 1)
    # the cap, by the check alone: nothing is staged for a hypothesis this long
    x = np.zeros((9, 29))
    with pytest.raises(ValueError, match="limit of %d" % LONG_MAX_LABELS):
        dec.score_long(x, tokens=[np.full(LONG_MAX_LABELS + 1, 2).tolist()])
    for name, bad in (("_tile_groups", 257), ("_tile_groups", -1), ("_tile_frames", 1.5), ("_budget", True)):
        with pytest.raises(ValueError, match=name):
            dec.score_long_batch([x], tokens=[[[2, 3]]], **{name: bad})
    for stream in (object.__new__(_DeviceStreams), list.__new__(_ResidentBeams)):
        with pytest.raises(NotImplementedError):
            dec.score_long(stream, tokens=[[2, 3]])
        with pytest.raises(NotImplementedError):
            dec.score_long_batch([stream], tokens=[[[2, 3]]])
    with pytest.raises(NotImplementedError):
        score_long_batch_sharded(dec, [x], [["a"]])
    with DevicePool(dec, devices=[0], library=sim_library.path) as pool:
        with pytest.raises(NotImplementedError):
            pool.score_long_batch([x], [["a"]])
    assert dec.score_long(x, ["ab"])[0].logp == dec.score(x, ["ab"])[0].logp


def test_native_call_validates_what_it_indexes_with(sim_library):  # noqa: F811
    """The C entry point on its own: error codes before anything is launched, and what it reports of a call."""
    dec = build(5)
    blank = dec._alphabet.labels.index("")
    x = np.zeros((4, 5))
    dll = dec._lib.dll
    i32p, i64p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)

    def call(target, frames=4, off=None, budget=0, groups=0, tile=0, out=True, logits=True):
        ptrs = (C.c_void_p * 1)(x.ctypes.data if logits else None)
        t = np.array(target or [0], dtype=np.int32)
        o = np.array(off or [0, len(target)], dtype=np.int64)
        logp, counts, plan = (C.c_double * 1)(), (C.c_int64 * 5)(), (C.c_int64 * 5)()
        rc = dll.ctcdec_score_long_batch(dec._handle, ptrs, (C.c_int32 * 1)(frames), 1, 1, 0, t.ctypes.data_as(i32p),
                                         o.ctypes.data_as(i64p), (C.c_int64 * 2)(0, 1), budget, groups, tile,
                                         C.cast(logp, f64p) if out else None, None, counts, plan)
        return rc, list(counts), list(plan)

    assert call([2, 3]) == (0, [1, 1, 1, 1, 1], [256, 4, 1, 1, 64])
    assert call([2, 3], groups=1, tile=3) == (0, [3, 4, 1, 1, 2], [1, 3, 2, 2, 64 + 24 * 3])
    assert call([2, 3, 2, 3, 2])[1] == [0, 0, 0, 0, 0]  # (needs five frames: -inf by the host, nothing launched)
    assert call([2, 5])[0] == -1 and call([-1])[0] == -1 and call([blank])[0] == -1
    assert call([2, 3], logits=False)[0] == -1 and call([2, 3], out=False)[0] == -1
    assert call([2, 3], off=[0, -1])[0] == -1 and call([2, 3], off=[1, 2])[0] == -1 and call([2, 3], frames=-1)[0] == -1
    assert call([2, 3], budget=-1)[0] == -1 and call([2, 3], groups=257)[0] == -1 and call([2, 3], tile=-1)[0] == -1
    # more labels than the cap: the offsets alone say so (the labels are never read)
    assert call([2], off=[0, LONG_MAX_LABELS + 1])[0] == -4
    assert b"utterance 0, hypothesis 0" in dll.ctcdec_last_error() and str(LONG_MAX_LABELS).encode() in dll.ctcdec_last_error()
    # a budget below the smallest plan: 2 labels, two state blocks of one group -- 64 bytes of column, 24 of edge row
    assert call([2, 3], groups=1, budget=88)[0] == 0 and call([2, 3], groups=1, budget=87)[0] == -4
    assert b"utterance 0, hypothesis 0" in dll.ctcdec_last_error() and b"88 bytes" in dll.ctcdec_last_error()
