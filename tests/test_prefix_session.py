"""Prefix sessions (prefix_session) on the CPU simulator of the kernels, which runs the body of ctc_prefix_advance
(csrc/ctc_align.h) child by child and the bodies of the stateless call as tests/test_prefix_scores.py does: the runners of
tests/prefix_session_util.py -- every prefix of a session against prefix_scores_batch of its labels with ==, a sample
against the numpy definition --, and the C entry points' own refusals. The HIP build: tests/test_gpu_prefix_session.py."""
import ctypes as C

import numpy as np
import pytest

from tests.align_util import random_logits
from tests.prefix_session_util import (run_arena, run_chain_identity, run_cost_contract, run_forward_boundary, run_independence,
                                       run_infeasible, run_label_limit, run_split_equals_fused, run_surface, run_tree_walk)
from tests.sim_util import sim_library  # noqa: F401
from tests.test_align import build

ERR_ARG, ERR_LIMIT = -1, -4  # CTCDEC_ERR_ARG, CTCDEC_ERR_LIMIT of include/ctcdec.h


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
@pytest.mark.parametrize("V", (29, 131))
def test_tree_walk_equals_the_stateless_call(V, dtype, sim_library):  # noqa: F811
    nodes = run_tree_walk(V=V, dtype=dtype)
    assert len(nodes) == 6 * (1 + 12 * 3)


def test_across_the_forward_kernel_boundary(sim_library, monkeypatch):  # noqa: F811
    run_forward_boundary(setenv=monkeypatch.setenv)


def test_infeasible_and_just_feasible_children(sim_library):  # noqa: F811
    run_infeasible()


def test_independence(sim_library):  # noqa: F811
    run_independence()


def test_split_and_fused_extensions(sim_library):  # noqa: F811
    few, _few_launches, _many_launches = run_split_equals_fused()
    assert len(few) == 5


def test_arena(sim_library):  # noqa: F811
    run_arena()


def test_longest_chain(sim_library):  # noqa: F811
    run_label_limit()


def test_cost_contract(sim_library):  # noqa: F811
    run_cost_contract(V=40, T=130)


def test_chain_identity(sim_library):  # noqa: F811
    run_chain_identity()


def test_surface(sim_library):  # noqa: F811
    dec = build(29)
    run_surface(dec)
    x = random_logits(np.random.default_rng(2), 10, 29)
    with dec.prefix_session([x, x[:4]]) as s:
        assert s.capacity == 128 and len(s) == 2 and s.last_next is None
        kid = s.extend([s.roots[1].id], texts=[" "])[0]
        assert kid.text == " " and kid.tokens == [1] and isinstance(kid.next_logp, np.ndarray) and kid.next_logp.shape == (29,)
        assert len(s.last_timing_ms) == 3 and len(s.last_launches) == 4
    with pytest.raises(ValueError, match="vocabulary"):
        dec.prefix_session([x[:, :5]])


def test_native_refusals(sim_library):  # noqa: F811
    """The C entry points check everything before anything is launched or taken, whatever the shell has checked before."""
    dll, dec = sim_library.dll, build(5)
    x = random_logits(np.random.default_rng(1), 6, 5)
    ptrs, frames = np.array([x.ctypes.data], dtype=np.uint64), np.array([6], dtype=np.int32)
    ids, end, nxt = np.zeros(4, dtype=np.int64), np.zeros(4), np.zeros((4, 5))
    i64, i32, f64 = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)

    def open_(capacity, frames=frames, next_dev=None, dtype=1):
        s = C.c_void_p()
        rc = dll.ctcdec_prefix_session_open(dec._handle, ptrs.ctypes.data_as(C.POINTER(C.c_void_p)), frames.ctypes.data_as(i32), 1, dtype, 0,
                                            capacity, next_dev, ids.ctypes.data_as(i64), end.ctypes.data_as(f64),
                                            C.c_void_p(nxt.ctypes.data), C.byref(s))
        return rc, s

    assert open_(0)[0] == ERR_ARG and open_(1 << 31)[0] == ERR_LIMIT and open_(2, dtype=7)[0] == ERR_ARG
    assert open_(2, frames=np.array([-1], dtype=np.int32))[0] == ERR_ARG
    assert open_(2, next_dev=C.c_void_p(nxt.ctypes.data))[0] == ERR_ARG  # (a buffer for next is device memory)
    rc, s = open_(3)
    assert rc == 0
    root = int(ids[0])

    def extend(parents, labels):
        par, lab = np.asarray(parents, dtype=np.int64), np.asarray(labels, dtype=np.int32)
        return dll.ctcdec_prefix_session_extend(s, par.ctypes.data_as(i64), lab.ctypes.data_as(i32), len(par), None,
                                                ids.ctypes.data_as(i64), end.ctypes.data_as(f64), C.c_void_p(nxt.ctypes.data))

    def release(which):
        arr = np.asarray(which, dtype=np.int64)
        return dll.ctcdec_prefix_session_release(s, arr.ctypes.data_as(i64), len(arr))

    try:
        for bad in (0, 5, -1):
            assert extend([root], [bad]) == ERR_ARG
        assert extend([root + 1], [2]) == ERR_ARG and extend([-1], [2]) == ERR_ARG and extend([root + (1 << 31)], [2]) == ERR_ARG
        assert extend([root] * 3, [2, 3, 4]) == ERR_LIMIT and b"free slots" in dll.ctcdec_last_error()
        assert extend([root, root], [2, 3]) == 0  # (the refusals took nothing)
        a, b = int(ids[0]), int(ids[1])
        assert np.isfinite(end[:2]).all() and np.isfinite(nxt[:2, 1:]).all() and np.isneginf(nxt[:2, 0]).all()
        assert release([root]) == ERR_ARG and release([a, a]) == ERR_ARG and release([b, root]) == ERR_ARG
        assert extend([a], [2]) == ERR_LIMIT  # (nothing was released)
        assert release([b]) == 0 and release([b]) == ERR_ARG and extend([b], [2]) == ERR_ARG
        assert extend([a], [2]) == 0 and int(ids[0]) != b  # (b's slot under a new id)
        ms, launches = (C.c_double * 3)(), (C.c_int32 * 4)()
        assert dll.ctcdec_prefix_session_timing(s, ms, launches) == 0 and tuple(launches)[2:] == (0, 0)
        assert dll.ctcdec_prefix_session_timing(None, ms, launches) == ERR_ARG
    finally:
        dll.ctcdec_prefix_session_close(s)
    dll.ctcdec_prefix_session_close(None)
