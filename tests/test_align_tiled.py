"""Tiled forced alignment of long transcripts (align_long(tiled=True)) on the CPU simulator of the kernels, which runs the
bodies of ctc_viterbi_tile and ctc_viterbi_cone (csrc/ctc_align.h) themselves with a one-thread context: every shape case of
tests/align_util.py equal to align bit for bit at every tile shape, targets above align's 2047 labels equal to align_long and
right against the numpy Viterbi, a span across a segment boundary, mixed batches, budgets, plans and the refusals in Python and
through the C entry point. The HIP build: tests/test_gpu_align_tiled.py."""
import ctypes as C

import numpy as np
import pytest

from tests.align_long_util import SHAPES, build, case_input, crosses, mixed_batch
from tests.align_tiled_util import ABOVE, check_above, check_equals_align, check_mixed_batch, tiled
from tests.align_util import SCORE_TOL
from tests.sim_util import sim_library  # noqa: F401


@pytest.mark.parametrize("case", SHAPES, ids=[c[0] for c in SHAPES])
def test_equals_align_at_every_tile_shape(case, sim_library):  # noqa: F811
    name, V, _T, target, _dtype, _kind = case
    dec = build(V)
    x = case_input(case)
    check_equals_align(dec, x, target, name)
    if name.endswith("_T300"):  # a label's span on both sides of a segment boundary: segments of 7 frames
        assert crosses(tiled(dec, [x], [target], (3, 7, 1))[0], 7), name


@pytest.mark.parametrize("case", ABOVE, ids=[c[0] for c in ABOVE])
def test_above_2047_labels_equals_align_long_and_numpy(case, sim_library):  # noqa: F811
    """Largest |score - numpy optimum| seen: 0 in all four cases, under the float64 SCORE_TOL = 1e-9 ("Forced
    alignment of long transcripts, tiled")."""
    assert check_above(build(case[1]), case) <= SCORE_TOL


def test_mixed_batch_and_budgets(sim_library):  # noqa: F811
    dec = build(29)
    xs, targets, bad = mixed_batch()
    most = check_mixed_batch(dec, xs)
    with pytest.raises(ValueError, match=r"utterance 3 .*without tiled needs less.* %d bytes" % most):
        tiled(dec, xs, targets, strict=False, _bp_budget=most - 1)
    with pytest.raises(ValueError, match=r"\[%d\]" % bad):
        tiled(dec, xs, targets)


@pytest.mark.parametrize("T,L", [(0, 0), (1, 1), (12, 12), (300, 129), (2300, 2049), (180000, 40000)])
def test_plans_agree(T, L, sim_library):  # noqa: F811
    """_align_tiled_plan is the native align_tiled_plan: the hour of the issue plans K = 448, 402 segments, about 257 MB"""
    dec = build(5)
    plan = dec._align_tiled_plan
    if (T, L) == (180000, 40000):
        assert plan(T, L, 1 << 30, 0, 0, 0) == (256, 64, 79, 2813, 7, 8 * (4 * 20001 + 3 * 78 * 64) + 32 * 20001 * 401, 448, 402)
        return
    rng = np.random.default_rng(T)
    x, target = rng.standard_normal((T, 5)), [2 + (k % 3) for k in range(L)]
    for cut in ((0, 0, 0), (3, 5, 2), (100, 97, 2)):
        tiled(dec, [x], [target], cut)
        assert dec.last_align_tiled_plan == [plan(T, L, 1 << 30, *cut)[:6]] and dec.last_align_long_plan == [plan(T, L, 1 << 30, *cut)[6:]]


def test_bad_arguments(sim_library):  # noqa: F811
    dec = build(5)
    x, target = np.zeros((9, 5)), [2, 3]
    good = dec.align(x, tokens=target)
    for kw in ({"_segment_frames": 2, "tiled": True}, {"_tile_groups": 2}, {"_tile_frames": 2}, {"_segment_blocks": 2},
               {"tiled": True, "_tile_groups": 257}, {"tiled": True, "_tile_frames": -1}, {"tiled": True, "_segment_blocks": 1.5},
               {"tiled": 1}, {"tiled": True, "_tile_frames": 5, "_segment_blocks": 90}):  # (the last: segments of 450 frames)
        with pytest.raises(ValueError):
            dec.align_long_batch([np.zeros((900, 5))], tokens=[target], **kw)
    assert dec.align_long(x, tokens=target, tiled=True).score == good.score
    # the C entry point on its own: codes before anything is launched
    dll, i32p, i64p = dec._lib.dll, C.POINTER(C.c_int32), C.POINTER(C.c_int64)

    def call(frames=9, budget=0, cut=(0, 0, 0), labels=(2, 3)):
        t, o = np.array(labels, dtype=np.int32), np.array([0, len(labels)], dtype=np.int64)
        res = C.c_void_p()
        rc = dll.ctcdec_align_tiled_batch(dec._handle, (C.c_void_p * 1)(x.ctypes.data), (C.c_int32 * 1)(frames), 1, 1, 0,
                                          t.ctypes.data_as(i32p), o.ctypes.data_as(i64p), 0, budget, *cut, C.byref(res))
        if rc == 0:
            dll.ctcdec_alignment_free(res)
        return rc

    assert call() == 0 and call(cut=(256, 9, 49)) == 0  # (FB is clamped to the 9 frames: segments of 441)
    assert call(cut=(257, 0, 0)) == -1 and call(cut=(-1, 0, 0)) == -1 and call(cut=(0, -1, 0)) == -1 and call(cut=(0, 0, -1)) == -1
    assert call(cut=(0, 9, 50)) == -1 and b"450 frames" in dll.ctcdec_last_error()
    assert call(labels=(2, 7)) == -1 and call(frames=-1) == -1 and call(budget=-1) == -1 and call(labels=(2, 2, 2, 2, 2, 2)) == -1
    # 9 frames, 2 labels: nch = 2, one segment -- a column of 64 bytes
    assert call(budget=64) == 0 and call(budget=63) == -4
    assert b"utterance 0" in dll.ctcdec_last_error() and b"64 bytes" in dll.ctcdec_last_error() and b"without tiled" in dll.ctcdec_last_error()
