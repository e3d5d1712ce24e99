"""GPU (-m gpu): CTC prefix scores (prefix_scores / prefix_scores_batch) on the HIP build -- ctc_forward_ends,
ctc_forward_wave_ends, ctc_prefix_extend and ctc_prefix_finish of csrc/ctc_align_hip.hip. The cases of
tests/test_prefix_scores.py from host arrays and from device tensors; frame counts around the segment length at vocabularies
of one and of several column tiles (131: rows off a 16-byte boundary); device tensors of every dtype read in place, one
through a view one element past an aligned base; label counts at the wave / group / 1024-thread edges under both forward
kernels; 1, K and K + 1 prefixes per utterance; split against unsplit launches; logp_end equal to score's float; next_logp
as views of one device tensor; the cost contract from the call's own timers; and every case against the CPU simulator."""
import numpy as np
import pytest
import torch

from tests.align_util import random_logits, random_target
from tests.prefix_util import PREFIX_K, PREFIX_SEG, check_prefix, close_prefix, next_array, same_prefix
from tests.score_util import shape_cases
from tests.test_align import build
from tests.test_prefix_scores import (BLANK, mixed_inputs, run_batch_equals_single_calls, run_chain_identity, run_chunks_of_k,
                                      run_edge_cases, run_score_identity, run_shape_case, run_split_equals_unsplit)

pytestmark = pytest.mark.gpu

SHAPES = shape_cases()
TORCH_DTYPES = (torch.float16, torch.bfloat16, torch.float32, torch.float64)
FRAMES = (1, PREFIX_SEG - 1, PREFIX_SEG, PREFIX_SEG + 1, 2 * PREFIX_SEG + 1)
VOCABS = (29, 131, 1024)
LABEL_EDGES = (0, 1, 2, 127, 128, 511, 512)  # the wave kernel's last, the group kernel's first, 256 threads' last, 1024's first


def on_device(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host_of(t):
    """A device tensor as the yardstick sees it: the exact values, in float64 for float64 and in float32 otherwise."""
    host = t.double().cpu().numpy()
    return host if t.dtype == torch.float64 else host.astype(np.float32)


@pytest.mark.parametrize("case", SHAPES, ids=[c[0] for c in SHAPES])
def test_shape_cases(case):
    host = run_shape_case(case)
    dev = run_shape_case(case, on_device)
    assert all(same_prefix(a, b) for a, b in zip(host, dev))


def run_frames_and_vocabularies(T, V, put=on_device):
    dec = build(V)
    rng = np.random.default_rng(1000 * V + T)
    x = random_logits(rng, T, V).astype(np.float32)
    prefixes = [[], [5], [5, 5], random_target(rng, 4, V)]
    got = dec.prefix_scores(put(x), tokens=prefixes)
    scored = dec.score(put(x), tokens=prefixes)
    for p, g, s in zip(prefixes, got, scored):
        assert g.logp_end == s.logp, (T, V, p)
        check_prefix(g, x, p, BLANK, "T=%d V=%d %s" % (T, V, p))
    return got


@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("T", FRAMES)
def test_frames_around_the_segment_length(T, V):
    dev = run_frames_and_vocabularies(T, V)
    host = run_frames_and_vocabularies(T, V, lambda x: x)
    assert all(same_prefix(a, b) for a, b in zip(dev, host))


@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("dtype", TORCH_DTYPES, ids=str)
def test_device_tensors(dtype, V):
    """Rows of every dtype read in place, in one batch: 1, K and K + 1 prefixes per utterance, and a view whose base is one
    element past an aligned address."""
    dec = build(V)
    rng = np.random.default_rng(V)
    xs = [torch.from_numpy(random_logits(rng, T, V)).to(dtype).cuda() for T in (37, PREFIX_SEG + 2, 5)]
    flat = torch.from_numpy(random_logits(rng, 20 * V + 1, 1)[:, 0]).to(dtype).cuda()
    xs.append(flat[1:].view(20, V))  # (contiguous, but its base is one element past an aligned address)
    counts = (1, PREFIX_K, PREFIX_K + 1, 2)
    prefixes = [[random_target(rng, 1 + k % 3, V, doubled=0) for k in range(n)] for n in counts]
    got = dec.prefix_scores_batch(xs, tokens=prefixes)
    for u, (x, ps) in enumerate(zip(xs, prefixes)):
        ref = host_of(x)
        assert len(got[u]) == counts[u]
        for j in sorted({0, len(ps) - 1}):
            check_prefix(got[u][j], ref, ps[j], BLANK, "%s V=%d utt %d prefix %d" % (dtype, V, u, j))
            assert same_prefix(got[u][j], dec.prefix_scores(x, tokens=[ps[j]])[0]), (dtype, V, u, j)


def run_label_edges(L, put=on_device):
    """T just above the fewest frames the prefix takes: the window's lower edge is active in every frame."""
    V = 29
    dec = build(V)
    rng = np.random.default_rng(L)
    p = random_target(rng, L, V, doubled=min(3, max(0, L - 1))) if L else []
    need = L + sum(1 for a, b in zip(p, p[1:]) if a == b)
    x = random_logits(rng, need + 3, V)
    xin = put(x)
    g = dec.prefix_scores(xin, tokens=[p])[0]
    assert g.logp_end == dec.score(xin, tokens=[p])[0].logp, L
    check_prefix(g, x, p, BLANK, "L=%d" % L)
    assert np.isfinite(next_array(g)[1:]).all()
    return g, dec.last_prefix_launched


@pytest.mark.parametrize("L", LABEL_EDGES)
def test_label_count_edges_under_both_forward_kernels(L, monkeypatch):
    plain, launched = run_label_edges(L)
    assert launched == ((1, 0) if L <= 127 else (0, 1))
    monkeypatch.setenv("CTCDEC_FORWARD_KERNEL", "group")
    forced, launched = run_label_edges(L)
    assert launched == (0, 1) and same_prefix(plain, forced), L  # (next_logp too: the end states have the same bits)
    monkeypatch.setenv("CTCDEC_FORWARD_KERNEL", "wave")
    wave, launched = run_label_edges(L)
    assert launched == ((1, 0) if L <= 127 else (0, 1)) and same_prefix(plain, wave), L


def test_logp_end_is_score():
    host = run_score_identity()
    dev = run_score_identity(on_device)
    assert all(same_prefix(a, b) for a, b in zip(host, dev))


def test_chain_identity():
    run_chain_identity(on_device)


def test_edge_cases():
    host = run_edge_cases()
    dev = run_edge_cases(on_device)
    assert all(same_prefix(a, b) for a, b in zip(host, dev))


@pytest.mark.parametrize("V", (29, 131))
def test_probabilities_and_logits_in_one_batch(V):
    for dtype in (np.float32, np.float64):
        xs = mixed_inputs(V, dtype, frames=(9, PREFIX_SEG + 30, 17, 1))
        host = run_batch_equals_single_calls(xs=xs, V=V)
        dev = run_batch_equals_single_calls(on_device, xs, V)
        assert all(same_prefix(a, b) for a, b in zip(host, dev))


@pytest.mark.parametrize("V", VOCABS)
def test_k_and_k_plus_1_prefixes(V):
    run_chunks_of_k(on_device, V, counts=(1, PREFIX_K, PREFIX_K + 1))


def test_split_and_unsplit_launches():
    """Three segments and two column tiles: 4096 prefixes make a launch that is not split."""
    few = run_split_equals_unsplit(on_device, V=300, T=2 * PREFIX_SEG + 1)
    host = run_split_equals_unsplit(V=300, T=2 * PREFIX_SEG + 1)
    assert all(same_prefix(a, b) for a, b in zip(few, host))


def test_next_logp_is_a_view_of_one_device_tensor():
    dec = build(131)
    rng = np.random.default_rng(3)
    xs = [on_device(random_logits(rng, T, 131).astype(np.float32)) for T in (40, 0, 3)]
    prefixes = [[[2, 3], []], [[], [4]], [[5, 6, 7, 8], [9]]]  # (the third utterance's first prefix has no path)
    got = dec.prefix_scores_batch(xs, tokens=prefixes)
    block = dec.last_prefix_next
    assert isinstance(block, torch.Tensor) and block.is_cuda and block.dtype == torch.float64 and tuple(block.shape) == (6, 131)
    h = 0
    for per_utt in got:
        for g in per_utt:
            assert isinstance(g.next_logp, torch.Tensor) and g.next_logp.device == xs[0].device and g.next_logp.dtype == torch.float64
            assert g.next_logp.untyped_storage().data_ptr() == block.untyped_storage().data_ptr()
            assert g.next_logp.data_ptr() == block[h].data_ptr() and tuple(g.next_logp.shape) == (131,)
            h += 1
    # the rows nothing was launched for are -inf on the device too
    assert got[1][0].logp_end == 0.0 and got[1][1].logp_end == -np.inf and got[2][0].logp_end == -np.inf
    for g in (got[1][0], got[1][1], got[2][0]):
        assert bool(torch.isneginf(g.next_logp).all())
    assert dec.last_prefix_launched == (3, 0)
    dec.prefix_scores(xs[0].cpu().numpy(), tokens=[[2]])
    assert dec.last_prefix_next is None


def test_cost_contract():
    """An utterance with 8 prefixes: row_lse is launched once, the forward pass and the extension both report time, and the
    launches are counted -- one forward launch, ctc_prefix_extend and (a split launch) ctc_prefix_finish."""
    dec = build(300)
    rng = np.random.default_rng(1)
    x = on_device(random_logits(rng, 500, 300).astype(np.float32))
    prefixes = [random_target(rng, 3 + k, 300) for k in range(8)]
    dec.prefix_scores(x, tokens=prefixes)
    ms, launches = dec.last_prefix_timing_ms, dec.last_prefix_launches
    print("8 prefixes: ms", ms, "launches", launches, "launched", dec.last_prefix_launched)
    assert len(ms) == 5 and all(v > 0.0 for v in ms)
    assert launches == (1, 1, 2) and dec.last_prefix_launched == (8, 0)
    dec.prefix_scores(x, tokens=prefixes + [random_target(rng, 200, 300)])
    print("9 prefixes, one long: launches", dec.last_prefix_launches)
    assert dec.last_prefix_launches == (1, 2, 2) and dec.last_prefix_launched == (8, 1)


def test_results_equal_the_simulator(monkeypatch):
    """The cases above on the HIP build and on the CPU simulator: finite values within 1e-9 (the two builds' exp and log
    differ in the last bits), -inf in the same places."""
    from pyctcdecode_amd import _binding as B
    from tests.sim.build_sim import build as build_sim

    def run_all():
        out = []
        for case in SHAPES:
            out += run_shape_case(case)
        for T in FRAMES:
            for V in (29, 131):
                out += run_frames_and_vocabularies(T, V, lambda x: x)
        out += run_frames_and_vocabularies(PREFIX_SEG + 1, 1024, lambda x: x)
        for L in LABEL_EDGES:
            out.append(run_label_edges(L, lambda x: x)[0])
        out += run_score_identity() + run_chain_identity() + run_edge_cases() + run_batch_equals_single_calls()
        out += run_chunks_of_k(V=131)
        return out

    hip = run_all()
    monkeypatch.setattr(B, "_LIB", B.Library(build_sim()))
    sim = run_all()
    assert len(hip) == len(sim) > 150
    for k, (a, b) in enumerate(zip(hip, sim)):
        assert close_prefix(a, b), (k, a.tokens, a.logp_end, b.logp_end)
