"""Alignment with gaps of long transcripts (align_gaps_long / align_gaps_long_batch) on the CPU simulator of the kernels, which
runs the body of ctc_viterbi_gaps_long (csrc/ctc_align.h) itself with a one-thread context: equal to align_gaps bit for bit at
every cut, the tie rule across a segment boundary, gap-free targets equal to align_long above 2047 labels, gapped targets above
2047 labels against numpy, a mixed batch over budgets, and the refusals. The HIP build: tests/test_gpu_align_gaps_long.py."""
import ctypes as C

import numpy as np
import pytest

from tests.align_gaps_long_util import (ABOVE, BATCH_PLUS_ONE, CASES, GAPPED_RUNS, SCORE_TOL, build, run_batch_plus_one_with_gaps,
                                        run_equals_align_gaps, run_gap_free_equals_align_long, run_gapped_above, run_mixed_batch,
                                        run_ties_across_a_boundary)
from tests.sim_util import sim_library  # noqa: F401


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_equals_align_gaps_at_every_cut(case, monkeypatch, sim_library):  # noqa: F811
    run_equals_align_gaps(case, monkeypatch)


@pytest.mark.parametrize("K", [1, 2, 3])
def test_tie_rule_across_a_boundary(K, sim_library):  # noqa: F811
    run_ties_across_a_boundary(K)


@pytest.mark.parametrize("case", ABOVE[:2] + [BATCH_PLUS_ONE], ids=lambda c: c[0])
def test_gap_free_equals_align_long_above_2047_labels(case, sim_library):  # noqa: F811
    run_gap_free_equals_align_long(case)


@pytest.mark.parametrize("case,pattern", GAPPED_RUNS, ids=["%s_%s" % (c[0], p) for c, p in GAPPED_RUNS])
def test_gaps_above_2047_labels_against_numpy(case, pattern, sim_library):  # noqa: F811
    """Largest |score - numpy optimum| seen: 0 in all five cases, under the float64 SCORE_TOL = 1e-9."""
    assert run_gapped_above(case, pattern) <= SCORE_TOL


def test_one_group_more_than_a_batch_with_every_slot_a_gap(sim_library):  # noqa: F811
    run_batch_plus_one_with_gaps()


def test_mixed_batch_budgets_and_refusals(sim_library):  # noqa: F811
    run_mixed_batch()
    dec = build(5)
    x = np.zeros((9, 5))
    with pytest.raises(ValueError, match=r"utterance 0 .* %d bytes" % dec._align_long_plan(9, 2, 1, 0)[2]):
        dec.align_gaps_long_batch([x], tokens=[[-1, 2, 3]], _bp_budget=dec._align_long_plan(9, 2, 1, 0)[2] - 1)
    with pytest.raises(ValueError, match="limit of 1048575"):
        dec._gapped_targets("align_gaps_long", [x], None, [np.full(1048576, 2)], "*", 1048575)
    with pytest.raises(ValueError, match="no label"):
        dec.align_gaps_long(x, tokens=[-1])
    # the C entry point: codes before anything is launched, and the gaps and the plan of a result
    dll, i32p, i64p = dec._lib.dll, C.POINTER(C.c_int32), C.POINTER(C.c_int64)

    def call(target, segment=0):
        t, o, res = np.array(target, dtype=np.int32), np.array([0, len(target)], dtype=np.int64), C.c_void_p()
        rc = dll.ctcdec_align_gaps_long_batch(dec._handle, (C.c_void_p * 1)(x.ctypes.data), (C.c_int32 * 1)(9), 1, 1, 0,
                                              t.ctypes.data_as(i32p), o.ctypes.data_as(i64p), 0, 0, segment, C.byref(res))
        return rc, res

    assert call([-1, 2, 3], segment=-1)[0] == -1 and call([-1])[0] == -1 and call([-1, -1, 2])[0] == -1
    assert call(np.full(1048576, 2))[0] == -4 and b"utterance 0" in dll.ctcdec_last_error()
    rc, res = call([-1, 2, 3], segment=4)
    go, gs, ge, n, sf, ns = i64p(), i32p(), i32p(), C.c_int64(), i32p(), i32p()
    lp = C.POINTER(C.c_double)()
    assert rc == 0 and dll.ctcdec_alignment_gaps(res, C.byref(go), C.byref(gs), C.byref(ge), C.byref(lp), C.byref(n)) == 0
    assert n.value == 1 and gs[0] == 0 and go[1] == 1
    assert dll.ctcdec_alignment_plan(res, C.byref(sf), C.byref(ns), C.byref(n)) == 0 and (sf[0], ns[0]) == (4, 2)
    dll.ctcdec_alignment_free(res)

    # streams, pools and ranks: not built
    from pyctcdecode_amd.decoder import _DeviceStreams
    from pyctcdecode_amd.parallel import DevicePool, align_gaps_long_batch_sharded

    stream = object.__new__(_DeviceStreams)
    for refused in (lambda: dec.align_gaps_long(stream, tokens=[2]), lambda: dec.align_gaps_long_batch([stream], tokens=[[2]]),
                    lambda: align_gaps_long_batch_sharded(dec, [x], ["a"]), lambda: DevicePool.align_gaps_long(None, [x], ["* a"])):
        with pytest.raises(NotImplementedError):
            refused()
    assert dec.align_gaps_long(x, "* a").text == "* a"
