"""GPU (-m gpu): frame posteriors (posteriors / posteriors_batch) on the HIP build -- ctc_posteriors of
csrc/ctc_align_hip.hip. The shape cases of tests/test_posteriors.py against the same numpy forward-backward from host arrays
and device tensors, the forward score against score's float for float, device tensors of every dtype read in place, both
instantiations of the kernel, batches and split launches against single calls, a small call on a stale workspace, the
summaries without the dense table, and the HIP build against the CPU simulator."""
import numpy as np
import pytest
import torch

from tests.posteriors_util import GAMMA_TOL, SCORE_TOL, check_posteriors, same_bits, window_mask, yardstick
from tests.score_util import case_input, random_logits, random_target, shape_cases
from tests.test_align import build, ragged_batch
from tests.test_posteriors import table_bytes

pytestmark = pytest.mark.gpu

SHAPES = shape_cases()
BY_NAME = {c[0]: c for c in SHAPES}


@pytest.mark.parametrize("case", SHAPES, ids=[c[0] for c in SHAPES])
def test_shape_cases(case):
    name, V, T, target, _dtype, _kind = case
    dec = build(V)
    x = case_input(case)
    blank = dec._alphabet.labels.index("")
    want = yardstick(x, target, blank)
    a = dec.posteriors(x, tokens=target)  # (a host array: staged)
    b = dec.posteriors(torch.from_numpy(x).cuda(), tokens=target)  # (a device tensor: read in place)
    check_posteriors(a, want, T, target, name + " host")
    check_posteriors(b, want, T, target, name + " device")
    assert same_bits(a, b)
    assert a.logp == dec.score(x, tokens=[target])[0].logp
    # 256 threads up to 511 labels (256 groups of states), 1024 above
    if name in ("L127_T300", "L128_T300", "L129_T300"):
        assert dec.last_posteriors_launched == (1, 0)
    if name == "limit_L2047":
        assert dec.last_posteriors_launched == (0, 1) and table_bytes(x, target) > 68e6


@pytest.mark.parametrize("V", [29, 131, 1024])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32, torch.float64])
def test_device_tensors(dtype, V):
    """The matrix of test_gpu_score.test_device_tensors, one target per utterance: rows of every dtype, at vocabularies whose
    rows are and are not 16-byte aligned, and a view whose base is one element past an aligned address."""
    dec = build(V)
    blank = dec._alphabet.labels.index("")
    rng = np.random.default_rng(V)
    xs, targets = [], []
    for T, L in ((37, 9), (64, 30), (5, 2)):
        xs.append(torch.from_numpy(random_logits(rng, T, V)).to(dtype).cuda())
        targets.append(random_target(rng, L, V, doubled=1))
    flat = torch.from_numpy(random_logits(rng, 20 * V + 1, 1)[:, 0]).to(dtype).cuda()
    xs.append(flat[1:].view(20, V))  # (contiguous, but its base is one element past an aligned address)
    targets.append(random_target(rng, 6, V))
    got = dec.posteriors_batch(xs, tokens=targets)
    for u, (x, t) in enumerate(zip(xs, targets)):
        host = x.double().cpu().numpy()
        ref = host if dtype == torch.float64 else host.astype(np.float32)  # (the widened values are exact)
        check_posteriors(got[u], yardstick(ref, t, blank), len(host), t, "%s V=%d utt %d" % (dtype, V, u))


def test_batch_equals_singles_and_split_launches():
    dec = build(29)
    xs, targets = ragged_batch()
    dev = [torch.from_numpy(x).cuda() for x in xs]
    batch = dec.posteriors_batch(dev, tokens=targets)
    assert dec.last_posteriors_launches == 1
    for u, t in enumerate(targets):
        assert same_bits(batch[u], dec.posteriors(dev[u], tokens=t)), u
    sizes = [table_bytes(x, t) for x, t in zip(xs, targets)]
    split = dec.posteriors_batch(dev, tokens=targets, _table_budget=max(max(sizes), sum(sizes) // 3))
    assert dec.last_posteriors_launches >= 3
    assert all(same_bits(a, b) for a, b in zip(split, batch))
    lean = dec.posteriors_batch(dev, tokens=targets, dense=False)
    assert all(b.gamma is None and same_bits(a, b, dense=False) for a, b in zip(batch, lean))
    # one call, both instantiations: the short targets in one launch, the long one in another
    rng = np.random.default_rng(3)
    x = random_logits(rng, 700, 29)
    mixed = [random_target(rng, L, 29, doubled=min(2, L // 2)) for L in (3, 511, 512, 40)]
    got = dec.posteriors_batch([x] * 4, tokens=mixed, dense=False)
    assert dec.last_posteriors_launched == (3, 1) and dec.last_posteriors_launches == 2
    for t, g in zip(mixed, got):
        assert same_bits(g, dec.posteriors(x, tokens=t, dense=False), dense=False), len(t)
        assert abs(g.logp - g.logp_backward) <= SCORE_TOL and g.logp == dec.score(x, tokens=[t])[0].logp


def test_small_call_on_a_stale_workspace():
    large = BY_NAME["L129_T300"]
    dec = build(29)
    got = dec.posteriors(case_input(large), tokens=large[3])
    assert got.gamma.shape == (300, 259) and float(got.gamma.max()) > 0.5
    for name in ("T_eq_L_no_blanks", "aaa_at_bound"):
        case = BY_NAME[name]
        x = case_input(case)
        if case[1] != 29:
            x = np.concatenate([x, np.full((len(x), 29 - case[1]), -40.0)], axis=1)
        stale, fresh = dec.posteriors(x, tokens=case[3]), build(29).posteriors(x, tokens=case[3])
        assert same_bits(stale, fresh), name
        assert (stale.gamma[~window_mask(*stale.gamma.shape)] == 0.0).all(), name
        check_posteriors(stale, yardstick(x, case[3], 0), len(x), case[3], name + " after a large call")


def test_hip_against_the_simulator(monkeypatch):
    from pyctcdecode_amd import _binding as B
    from tests.sim.build_sim import build as build_sim

    xs, targets = ragged_batch()
    hip = build(29).posteriors_batch(xs, tokens=targets)
    monkeypatch.setattr(B, "_LIB", B.Library(build_sim()))
    sim = build(29).posteriors_batch(xs, tokens=targets)
    worst_gamma = worst_logp = 0.0
    for u, (a, b) in enumerate(zip(hip, sim)):
        assert a.gamma.shape == b.gamma.shape, u
        if a.gamma.size:
            worst_gamma = max(worst_gamma, float(np.abs(a.gamma - b.gamma).max()))
        worst_logp = max(worst_logp, abs(a.logp - b.logp))
    print("HIP against the simulator: gamma %.2e, logp %.2e" % (worst_gamma, worst_logp))
    assert worst_gamma <= GAMMA_TOL and worst_logp <= SCORE_TOL
