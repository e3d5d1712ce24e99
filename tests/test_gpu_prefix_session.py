"""GPU (-m gpu): prefix sessions (prefix_session) on the HIP build -- ctc_prefix_advance of csrc/ctc_align_hip.hip in front
of the stateless call's ctc_prefix_extend. The runners of tests/prefix_session_util.py on device tensors and on host
arrays: every prefix of a session against prefix_scores_batch of its labels with ==, at vocabularies of one and of several
column tiles (1022: no multiple of 4), frame counts around the segment length and every dtype read in place; the chain across
the wave / group boundary of the stateless forward kernels; host input against device input; next_logp as views of the
step's one device tensor; and the cost contract from the call's own event logs."""
import numpy as np
import pytest
import torch

from tests.prefix_session_util import (FRAMES, run_arena, run_chain_identity, run_cost_contract, run_forward_boundary,
                                       run_independence, run_infeasible, run_label_limit, run_split_equals_fused, run_surface,
                                       run_tree_walk, same)
from tests.prefix_util import same_prefix
from tests.test_align import build
from tests.test_gpu_prefix_scores import host_of, on_device

pytestmark = pytest.mark.gpu

HALF = {"f16": torch.float16, "bf16": torch.bfloat16}


@pytest.mark.parametrize("dtype", (np.float64, np.float32), ids=("f64", "f32"))
@pytest.mark.parametrize("V", (29, 131, 1022, 1024))
def test_tree_walk_equals_the_stateless_call(V, dtype):
    dev = run_tree_walk(on_device, V=V, dtype=dtype)
    assert len(dev) == len(FRAMES) * (1 + 12 * 3)
    if V in (131, 1024):  # host arrays give the same bits
        host = run_tree_walk(same, V=V, dtype=dtype)
        assert all(same_prefix(a, b) for a, b in zip(dev, host))


@pytest.mark.parametrize("name", sorted(HALF))
@pytest.mark.parametrize("V", (131, 1024))
def test_tree_walk_in_half_precision(V, name):
    """Logits alone: a half-precision softmax row no longer sums to 1, and the numpy definition tells probabilities from
    logits by that sum."""
    run_tree_walk(lambda x: torch.from_numpy(x).to(HALF[name]).cuda(), V=V, dtype=np.float32, mixed=False, host_of=host_of)


def test_across_the_forward_kernel_boundary(monkeypatch):
    dev = run_forward_boundary(on_device, monkeypatch.setenv)
    monkeypatch.delenv("CTCDEC_FORWARD_KERNEL")
    host = run_forward_boundary(same, monkeypatch.setenv)
    assert all(same_prefix(a, b) for a, b in zip(dev, host))


def test_infeasible_and_just_feasible_children():
    dev, host = run_infeasible(on_device), run_infeasible()
    assert all(same_prefix(a, b) for a, b in zip(dev, host))


def test_independence():
    dev, host = run_independence(on_device), run_independence()
    assert all(same_prefix(a, b) for a, b in zip(dev, host))


def test_split_and_fused_extensions():
    """Three segments and two column tiles; 4096 children make an extension that is not split: one launch instead of two."""
    few, few_launches, many_launches = run_split_equals_fused(on_device, V=300, T=2 * 128 + 1)
    assert few_launches[:2] == (1, 2) and many_launches[:2] == (1, 1)
    host = run_split_equals_fused(V=300, T=2 * 128 + 1)[0]
    assert all(same_prefix(a, b) for a, b in zip(few, host))


def test_arena():
    run_arena(on_device)


def test_longest_chain():
    run_label_limit(on_device)


def test_cost_contract():
    opened, extend, ms, stateless = run_cost_contract(on_device)
    assert opened[0] == 0 and opened[2:] == (1, 1)  # (the session's one row_lse and the roots' forward pass)
    assert extend == (1, 2, 0, 0) and stateless == (1, 1, 2)
    assert ms[0] > 0.0 and ms[1] > 0.0 and ms[2] >= ms[0] + ms[1]


def test_chain_identity():
    run_chain_identity(on_device)


def test_surface():
    """next_logp rows are views of the step's one [n, V] tensor, which last_next exposes; rows of an utterance without
    frames are -inf on the device too."""
    dec = build(131)
    run_surface(dec)
    rng = np.random.default_rng(3)
    xs = [on_device(rng.standard_normal((T, 131)).astype(np.float32)) for T in (40, 0, 3)]
    with dec.prefix_session(xs) as s:
        for k in range(2):
            step = s.roots if k == 0 else s.extend([r.id for r in s.roots] + [s.roots[0].id], [5, 6, 7, 8])
            block = s.last_next
            assert isinstance(block, torch.Tensor) and block.is_cuda and block.dtype == torch.float64 and tuple(block.shape) == (len(step), 131)
            for h, g in enumerate(step):
                assert g.next_logp.untyped_storage().data_ptr() == block.untyped_storage().data_ptr()
                assert g.next_logp.data_ptr() == block[h].data_ptr() and tuple(g.next_logp.shape) == (131,)
        assert s.roots[1].logp_end == 0.0 and step[1].logp_end == -np.inf
        assert bool(torch.isneginf(step[1].next_logp).all()) and bool(torch.isfinite(step[3].next_logp[1:]).all())
        roots_block = s.roots[0].next_logp  # (a step's tensor lives as long as a view of it)
        assert bool(torch.isfinite(roots_block[1:]).all())
