"""GPU (-m gpu): transcript likelihood (score / score_batch) on the HIP build -- ctc_forward and ctc_forward_wave of
csrc/ctc_align_hip.hip. The shape and normalisation cases of tests/test_score.py against the same numpy forward recursion
from host arrays and device tensors, device tensors of every dtype read in place, the wave kernel against the group kernel
float for float, one call that launches both, and the HIP build against the CPU simulator."""
import math

import numpy as np
import pytest
import torch

from tests.score_util import (NORMALISATION, SCORE_TOL, WAVE_MAX_LABELS, all_sequences, case_input, feasible, neg_inf_case,
                              normalisation_input, random_logits, random_target, shape_cases, yardstick)
from tests.test_align import build, ragged_batch
from tests.test_score import check_score, ragged_hyps

pytestmark = pytest.mark.gpu

SHAPES = shape_cases()
SHORT = [c for c in SHAPES if len(c[3]) <= WAVE_MAX_LABELS and c[2] > 0]
LONG = [c for c in SHAPES if c[0] in ("L128_T300", "L129_T300")]


def logps(scored):
    return [g.logp for g in scored]


@pytest.mark.parametrize("case", SHAPES, ids=[c[0] for c in SHAPES])
def test_shape_cases(case):
    name, V, _T, target, _dtype, _kind = case
    dec = build(V)
    x = case_input(case)
    blank = dec._alphabet.labels.index("")
    want = yardstick(x, target, blank)
    a = dec.score(x, tokens=[target])[0].logp  # (a host array: staged)
    b = dec.score(torch.from_numpy(x).cuda(), tokens=[target])[0].logp  # (a device tensor: read in place)
    check_score(a, want, name + " host")
    check_score(b, want, name + " device")
    assert a == b


def test_no_frames_and_neg_inf_logits():
    dec = build(29)
    blank = dec._alphabet.labels.index("")
    got = dec.score(torch.zeros((0, 29), dtype=torch.float64).cuda(), tokens=[[2, 3], []])
    assert logps(got) == [-np.inf, 0.0] and dec.last_score_launched == (0, 0)
    x, target = neg_inf_case()
    a, b = dec.score(x, tokens=[target])[0].logp, dec.score(torch.from_numpy(x).cuda(), tokens=[target])[0].logp
    assert math.isfinite(a) and a == b
    check_score(a, yardstick(x, target, blank), "-inf logits")


@pytest.mark.parametrize("V,T,n_hyps,n_infeasible", NORMALISATION, ids=["V%d_T%d" % c[:2] for c in NORMALISATION])
def test_all_sequences_sum_to_one(V, T, n_hyps, n_infeasible):
    dec = build(V)
    blank = dec._alphabet.labels.index("")
    x = normalisation_input(V, T)
    seqs = all_sequences(V, T, blank)
    assert len(seqs) == n_hyps
    host = dec.score(x, tokens=seqs)
    dev = dec.score(torch.from_numpy(x).cuda(), tokens=seqs)
    assert logps(host) == logps(dev)
    assert sum(dec.last_score_launched) == n_hyps - n_infeasible
    for s, g in zip(seqs, host):
        if feasible(T, s):
            check_score(g.logp, yardstick(x, s, blank), str(s))
        else:
            assert g.logp == -np.inf, (s, g.logp)
    total = math.fsum(math.exp(g.logp) for g in host)
    print("V=%d T=%d: the probabilities of %d sequences sum to 1 %+.3e" % (V, T, n_hyps, total - 1.0))
    assert abs(total - 1.0) <= 1e-12, total


@pytest.mark.parametrize("V", [29, 131, 1024])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32, torch.float64])
def test_device_tensors(dtype, V):
    """The matrix of test_gpu_align.test_device_tensors, three hypotheses per utterance: rows of every dtype, at vocabularies
    whose rows are and are not 16-byte aligned, and a view whose base is one element past an aligned address."""
    dec = build(V)
    blank = dec._alphabet.labels.index("")
    rng = np.random.default_rng(V)
    xs, hyps = [], []
    for T, L in ((37, 9), (64, 30), (5, 2)):
        xs.append(torch.from_numpy(random_logits(rng, T, V)).to(dtype).cuda())
        t = random_target(rng, L, V, doubled=1)
        hyps.append([t, t[:-1], t[1:] + random_target(rng, 1, V)])
    flat = torch.from_numpy(random_logits(rng, 20 * V + 1, 1)[:, 0]).to(dtype).cuda()
    xs.append(flat[1:].view(20, V))  # (contiguous, but its base is one element past an aligned address)
    t = random_target(rng, 6, V)
    hyps.append([t, t[:3], []])
    got = dec.score_batch(xs, tokens=hyps)
    for u, (x, hs) in enumerate(zip(xs, hyps)):
        host = x.double().cpu().numpy()
        ref = host if dtype == torch.float64 else host.astype(np.float32)  # (the widened values are exact)
        for j, h in enumerate(hs):
            check_score(got[u][j].logp, yardstick(ref, h, blank), "%s V=%d utt %d hyp %d" % (dtype, V, u, j))


def test_wave_kernel_equals_group_kernel(monkeypatch):
    """Every case the wave kernel takes (L = 31, 32 and 127 put states across the lane and wave edges), under each kernel
    forced in turn: the floats are equal, and last_score_launched shows which kernel took them."""
    jobs = [(c[1], case_input(c), [c[3]], c[0]) for c in SHORT]
    for V, T, _n, _bad in NORMALISATION:
        blank = build(V)._alphabet.labels.index("")
        jobs.append((V, normalisation_input(V, T), all_sequences(V, T, blank), "all V=%d T=%d" % (V, T)))
    got = {}
    for kernel in ("wave", "group"):
        monkeypatch.setenv("CTCDEC_FORWARD_KERNEL", kernel)
        for V, x, seqs, name in jobs:
            dec = build(V)
            got[kernel, name] = logps(dec.score(x, tokens=seqs))
            n = sum(1 for s in seqs if feasible(len(x), s))
            assert dec.last_score_launched == ((n, 0) if kernel == "wave" else (0, n)), (kernel, name, dec.last_score_launched)
    for V, x, seqs, name in jobs:
        assert got["wave", name] == got["group", name], name
        blank = build(V)._alphabet.labels.index("")
        for s, g in zip(seqs, got["wave", name]):
            check_score(g, yardstick(x, s, blank), name)


def test_long_targets_take_the_group_kernel_under_wave(monkeypatch):
    monkeypatch.setenv("CTCDEC_FORWARD_KERNEL", "wave")
    assert len(LONG) == 2
    for c in LONG:
        dec = build(c[1])
        x = case_input(c)
        got = dec.score(x, tokens=[c[3]])[0].logp
        assert dec.last_score_launched == (0, 1)
        check_score(got, yardstick(x, c[3], dec._alphabet.labels.index("")), c[0])


def test_one_call_launches_both_kernels():
    dec = build(29)
    blank = dec._alphabet.labels.index("")
    rng = np.random.default_rng(6)
    x = random_logits(rng, 600, 29)
    hyps = [random_target(rng, L, 29, doubled=min(2, L // 2)) for L in (3, 127, 128, 40, 260, 0, 520)]
    got = logps(dec.score(torch.from_numpy(x).cuda(), tokens=hyps))
    assert dec.last_score_launched == (4, 3)
    for h, g in zip(hyps, got):
        assert dec.score(x, tokens=[h])[0].logp == g, len(h)
        check_score(g, yardstick(x, h, blank), "L=%d" % len(h))


def test_ragged_batch_equals_singles_and_the_simulator(monkeypatch):
    from pyctcdecode_amd import _binding as B
    from tests.sim.build_sim import build as build_sim

    dec = build(29)
    xs, targets = ragged_batch()
    hyps = ragged_hyps(targets)
    dev = [torch.from_numpy(x).cuda() for x in xs]
    batch = dec.score_batch(dev, tokens=hyps)
    for u, h in enumerate(hyps):
        assert logps(batch[u]) == logps(dec.score(dev[u], tokens=h)), u
    T = max(len(x) for x in xs)
    pad = np.zeros((len(xs), T, 29))
    for u, x in enumerate(xs):
        pad[u, : len(x)] = x
    cube = dec.score_batch(torch.from_numpy(pad).cuda(), tokens=hyps)
    for u, h in enumerate(hyps):
        assert logps(cube[u]) == logps(dec.score(pad[u], tokens=h)), u
    monkeypatch.setattr(B, "_LIB", B.Library(build_sim()))
    sim = build(29).score_batch(xs, tokens=hyps)
    worst = 0.0
    for u, (a, b) in enumerate(zip(batch, sim)):
        for p, q in zip(logps(a), logps(b)):
            if math.isinf(q):
                assert p == q, u
            else:
                worst = max(worst, abs(p - q))
                assert abs(p - q) <= SCORE_TOL, (u, p, q)
    print("HIP against the simulator: worst gap %.2e" % worst)
