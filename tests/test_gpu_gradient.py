"""GPU (-m gpu): the transcript gradient (gradient / gradient_batch / ctc_loss) on the HIP build -- ctc_grad_rows of
csrc/ctc_align_hip.hip behind a dense ctc_posteriors launch. The shape cases of tests/test_gradient.py against the same numpy
yardstick from host arrays and device tensors, bit-equal to each other; the clipped cases; device tensors of every dtype written
in place; batches, split launches, both ctc_posteriors instantiations and a [B, T, V] tensor against single calls; a repeated
call; a small call on a stale workspace; ctc_loss under autograd; and the HIP build against the CPU simulator."""
import numpy as np
import pytest
import torch

from tests.grad_util import (GRAD_TOL, SCORE_TOL, check_gradient, check_rows, clipped_target_case, grad_np, grad_torch,
                             neg_inf_case, same_bits, unclipped)
from tests.score_util import case_input, random_logits, random_target, shape_cases
from tests.test_align import build, ragged_batch
from tests.test_posteriors import table_bytes

pytestmark = pytest.mark.gpu

SHAPES = shape_cases()
BY_NAME = {c[0]: c for c in SHAPES}


def reference(x, target, V):
    return grad_np(x, target, 0) if len(x) else (0.0, np.zeros((0, V)))


@pytest.mark.parametrize("case", SHAPES, ids=[c[0] for c in SHAPES])
def test_shape_cases(case):
    name, V, T, target, _dtype, kind = case
    dec = build(V)
    x = case_input(case)
    want = reference(x, target, V)
    a = dec.gradient(x, tokens=target)  # (a host array: staged, the rows copied back)
    b = dec.gradient(torch.from_numpy(x).cuda(), tokens=target)  # (a device tensor: read and written in place)
    grad = check_gradient(a, want, x, target, name + " host")
    check_gradient(b, want, x, target, name + " device", on_device=True)
    assert same_bits(a, b)
    assert a.logp == dec.score(x, tokens=[target])[0].logp
    assert dec.last_gradient_launches == (2 if T > 0 else 0)
    if T > 0 and kind != "probs":
        check_rows(grad, x, target, 0, name)
    # ctc_posteriors: 256 threads up to 511 labels (256 groups of states), 1024 above
    if name in ("L127_T300", "L128_T300", "L129_T300"):
        assert dec.last_gradient_launched == (1, 0)
    if name == "limit_L2047":  # (about 680 states to each of the three labels: the long occurrence lists)
        assert dec.last_gradient_launched == (0, 1)
    assert same_bits(b, dec.gradient(torch.from_numpy(x).cuda(), tokens=target))  # (a repeated call on the same decoder)


@pytest.mark.parametrize("which", ["neg_inf", "clipped_target"])
def test_clipped_entries(which):
    V, (x, target), n_floor = (29, neg_inf_case(), 10) if which == "neg_inf" else (12, clipped_target_case(), 31)
    dec = build(V)
    want = grad_np(x, target, 0)
    a, b = dec.gradient(x, tokens=target), dec.gradient(torch.from_numpy(x).cuda(), tokens=target)
    grad = check_gradient(a, want, x, target, which + " host")
    check_gradient(b, want, x, target, which + " device", on_device=True)
    assert same_bits(a, b) and a.logp == dec.score(x, tokens=[target])[0].logp and np.isfinite(grad).all()
    # a clipped entry keeps no share of gamma: its gradient is -softmax * M alone, so not positive -- target label or not
    floor = ~unclipped(x)
    assert int(floor.sum()) == n_floor and (grad[floor] <= 0.0).all() and floor[:, target].any()


@pytest.mark.parametrize("V", [29, 131, 1024])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32, torch.float64])
def test_device_tensors(dtype, V):
    """The matrix of test_gpu_posteriors.test_device_tensors: rows of every dtype, at vocabularies that take each grouping of a
    row's threads (16 lanes, a wave, the workgroup) and whose rows are and are not 16-byte aligned, and a view whose base is one
    element past an aligned address. The gradients are views of one device allocation."""
    dec = build(V)
    rng = np.random.default_rng(V)
    xs, targets = [], []
    for T, L in ((37, 9), (64, 30), (5, 2)):
        xs.append(torch.from_numpy(random_logits(rng, T, V)).to(dtype).cuda())
        targets.append(random_target(rng, L, V, doubled=1))
    flat = torch.from_numpy(random_logits(rng, 20 * V + 1, 1)[:, 0]).to(dtype).cuda()
    xs.append(flat[1:].view(20, V))  # (contiguous, but its base is one element past an aligned address)
    targets.append(random_target(rng, 6, V))
    got = dec.gradient_batch(xs, tokens=targets)
    base = got[0].grad.untyped_storage().data_ptr()
    for u, (x, t) in enumerate(zip(xs, targets)):
        host = x.double().cpu().numpy()
        ref = host if dtype == torch.float64 else host.astype(np.float32)  # (the widened values are exact)
        grad = check_gradient(got[u], grad_np(ref, t, 0), ref, t, "%s V=%d utt %d" % (dtype, V, u), on_device=True)
        check_rows(grad, ref, t, 0, "%s V=%d utt %d" % (dtype, V, u))
        assert got[u].grad.device == x.device and got[u].grad.untyped_storage().data_ptr() == base
        assert same_bits(got[u], dec.gradient(x, tokens=t)), u


@pytest.mark.parametrize("V,dtype", [(64, np.float64), (65, np.float32), (256, np.float16), (257, np.float64), (1025, np.float32),
                                     (4100, np.float64), (4100, np.float16)])
def test_vocabulary_thresholds(V, dtype):
    """Either side of every size at which a row changes hands: 16 lanes up to 64 labels, a wave up to 256, the workgroup with
    four entries per thread up to 1024 and sixteen above, and past 4096 labels, where the entries a thread does not keep are
    formed in both passes. Two utterances, so that a workgroup of small rows spans both."""
    dec = build(V)
    rng = np.random.default_rng(V)
    xs = [random_logits(rng, T, V).astype(dtype) for T in (19, 7)]
    targets = [random_target(rng, 6, V, doubled=1), [V - 1, 2, V - 1]]
    host = dec.gradient_batch(xs, tokens=targets)
    dev = dec.gradient_batch([torch.from_numpy(x).cuda() for x in xs], tokens=targets)
    for u, (x, t) in enumerate(zip(xs, targets)):
        grad = check_gradient(host[u], grad_np(x, t, 0), x, t, "V=%d %s utt %d" % (V, np.dtype(dtype).name, u))
        check_rows(grad, x, t, 0, "V=%d utt %d" % (V, u))
        assert same_bits(host[u], dev[u]) and same_bits(host[u], dec.gradient(x, tokens=t)), (V, u)


def test_batch_equals_singles_and_split_launches():
    dec = build(29)
    xs, targets = ragged_batch()
    dev = [torch.from_numpy(x).cuda() for x in xs]
    batch = dec.gradient_batch(dev, tokens=targets)
    assert dec.last_gradient_launches == 2
    host = dec.gradient_batch(xs, tokens=targets)
    for u, t in enumerate(targets):
        assert same_bits(batch[u], dec.gradient(dev[u], tokens=t)), u
        assert same_bits(batch[u], host[u]), u
        check_gradient(host[u], reference(xs[u], t, 29), xs[u], t, "utt %d" % u)
    sizes = [table_bytes(x, t) for x, t in zip(xs, targets)]
    budget = max(max(sizes), sum(sizes) // 3)
    split = dec.gradient_batch(dev, tokens=targets, _table_budget=budget)
    assert dec.last_gradient_launches >= 6
    assert all(same_bits(a, b) for a, b in zip(split, batch))
    split_host = dec.gradient_batch(xs, tokens=targets, _table_budget=budget)
    assert all(same_bits(a, b) for a, b in zip(split_host, batch))
    # a padded [B, T, V] tensor against the list of its slices
    T = max(len(x) for x in xs)
    pad = torch.zeros((len(xs), T, 29), dtype=torch.float64, device="cuda")
    for u, x in enumerate(dev):
        pad[u, : len(x)] = x
    cube = dec.gradient_batch(pad, tokens=targets)
    for u, (g, s) in enumerate(zip(cube, dec.gradient_batch(list(pad), tokens=targets))):
        assert same_bits(g, s), u
    # one call, both ctc_posteriors instantiations: the short targets in one launch, the long one in another
    rng = np.random.default_rng(3)
    x = torch.from_numpy(random_logits(rng, 700, 29)).cuda()
    mixed = [random_target(rng, L, 29, doubled=min(2, L // 2)) for L in (3, 511, 512, 40)]
    got = dec.gradient_batch([x] * 4, tokens=mixed)
    assert dec.last_gradient_launched == (3, 1) and dec.last_gradient_launches == 3
    for t, g in zip(mixed, got):
        assert same_bits(g, dec.gradient(x, tokens=t)), len(t)
        assert g.logp == dec.score(x, tokens=[t])[0].logp
        check_gradient(g, grad_np(x.cpu().numpy(), t, 0), x.cpu().numpy(), t, "L=%d" % len(t), on_device=True)


def test_small_call_on_a_stale_workspace():
    large = BY_NAME["L129_T300"]
    dec = build(29)
    got = dec.gradient(case_input(large), tokens=large[3])
    assert got.grad.shape == (300, 29) and float(np.abs(got.grad).max()) > 0.5
    for name in ("T_eq_L_no_blanks", "aaa_at_bound"):
        case = BY_NAME[name]
        x = case_input(case)
        if case[1] != 29:
            x = np.concatenate([x, np.full((len(x), 29 - case[1]), -40.0)], axis=1)
        stale, fresh = dec.gradient(x, tokens=case[3]), build(29).gradient(x, tokens=case[3])
        assert same_bits(stale, fresh), name
        check_gradient(stale, grad_np(x, case[3], 0), x, case[3], name + " after a large call")


def test_refusals():
    from pyctcdecode_amd.parallel import gradient_batch_sharded

    dec = build(5)
    x = torch.zeros((9, 5), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match=r"no alignment for utterances \[1\]"):
        dec.gradient_batch([x, x[:2]], tokens=[[2, 3], [2, 2]])
    got = dec.gradient_batch([x, x[:2], x], tokens=[[2, 3], [2, 2], [3]], strict=False)
    assert got[1] is None and got[0].tokens == [2, 3] and tuple(got[2].grad.shape) == (9, 5) and got[2].grad.is_cuda
    with pytest.raises(ValueError, match="utterance 0 .*limit of 2047"):
        dec.gradient(torch.zeros((2100, 5), device="cuda"), tokens=random_target(np.random.default_rng(1), 2048, 5))
    for bad in ([0], [5], [-1]):
        with pytest.raises(ValueError, match=r"tokens\[0\].*label id"):
            dec.gradient(x, tokens=bad)
    with pytest.raises(NotImplementedError):
        gradient_batch_sharded(dec, [x], ["a"])
    with pytest.raises(ValueError, match="no alignment"):
        dec.ctc_loss([x[:2]], tokens=[[2, 2, 2]])
    with pytest.raises(ValueError, match="reduction"):
        dec.ctc_loss([x], tokens=[[2]], reduction="mean")


def test_ctc_loss_sum():
    """A float64 leaf, reduction="sum", an upstream factor of 0.5: x.grad is -0.5 * gradient_batch's grad, float for float, and
    agrees with torch's own ctc_loss under autograd."""
    dec = build(29)
    xs, targets = ragged_batch(n=6, seed=9)
    leaves = [torch.from_numpy(x).cuda().requires_grad_(True) for x in xs]
    loss = dec.ctc_loss(leaves, tokens=targets, reduction="sum")
    assert loss.dtype == torch.float64 and loss.shape == () and loss.is_cuda
    (0.5 * loss).backward()
    want = dec.gradient_batch([v.detach() for v in leaves], tokens=targets)
    scores = [dec.score(x, tokens=[t])[0].logp for x, t in zip(xs, targets)]
    assert abs(float(loss.detach()) + sum(scores)) <= 1e-12 * abs(sum(scores))  # (six exact negations, summed in the device's order)
    worst = 0.0
    for v, w, x, t in zip(leaves, want, xs, targets):
        assert v.grad.dtype == torch.float64 and v.grad.shape == v.shape
        assert torch.equal(v.grad, -0.5 * w.grad)
        if len(x):
            worst = max(worst, float(np.abs(-2.0 * v.grad.cpu().numpy() - grad_torch(x, t, 0)[1]).max()))
    print("ctc_loss against torch's ctc_loss under autograd: %.1e" % worst)
    assert worst <= GRAD_TOL


def test_ctc_loss_none_and_float32():
    dec = build(29)
    rng = np.random.default_rng(12)
    cube = torch.from_numpy(random_logits(rng, 3 * 40 * 29, 1).reshape(3, 40, 29))
    targets = [random_target(rng, L, 29, doubled=1) for L in (7, 12, 3)]
    weights = torch.tensor([1.0, -2.0, 0.25], dtype=torch.float64, device="cuda")
    for dtype in (torch.float64, torch.float32):
        leaf = cube.to(dtype).cuda().requires_grad_(True)
        loss = dec.ctc_loss(leaf, tokens=targets, reduction="none")
        assert loss.shape == (3,) and loss.dtype == torch.float64
        want = dec.gradient_batch(leaf.detach(), tokens=targets)
        assert loss.tolist() == [-dec.score(leaf.detach()[u], tokens=[targets[u]])[0].logp for u in range(3)]
        assert loss.tolist() == [-w.logp for w in want]
        (loss * weights).sum().backward()
        assert leaf.grad.dtype == dtype and leaf.grad.shape == leaf.shape
        for u in range(3):
            assert torch.equal(leaf.grad[u], (want[u].grad * -weights[u]).to(dtype)), (dtype, u)


def test_hip_against_the_simulator(monkeypatch):
    from pyctcdecode_amd import _binding as B
    from tests.sim.build_sim import build as build_sim

    xs, targets = ragged_batch()
    hip = build(29).gradient_batch(xs, tokens=targets)
    monkeypatch.setattr(B, "_LIB", B.Library(build_sim()))
    sim = build(29).gradient_batch(xs, tokens=targets)
    worst_grad = worst_logp = 0.0
    for u, (a, b) in enumerate(zip(hip, sim)):
        assert a.grad.shape == b.grad.shape and a.grad.dtype == b.grad.dtype, u
        if a.grad.size:
            worst_grad = max(worst_grad, float(np.abs(a.grad - b.grad).max()))
        worst_logp = max(worst_logp, abs(a.logp - b.logp))
    print("HIP against the simulator: grad %.2e, logp %.2e" % (worst_grad, worst_logp))
    assert worst_grad <= GRAD_TOL and worst_logp <= SCORE_TOL
