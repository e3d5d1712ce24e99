"""GPU (-m gpu): forced alignment (align / align_batch) on the HIP build -- row_lse and ctc_viterbi of
csrc/ctc_align_hip.hip. The shape cases and goldens of tests/test_align.py against the same numpy Viterbi, device tensors of
every dtype read in place, ragged batches through a list and a [B, T, V] tensor, a batch forced over a tiny back-pointer
budget into several launches, and paths equal to the CPU simulator's on inputs without score ties."""
import numpy as np
import pytest
import torch

from tests.align_util import FOLDS, case_input, check_aligned, random_logits, random_target, shape_cases
from tests.test_align import GOLDEN_NAMES, build, golden_case, overlaps, ragged_batch, same

pytestmark = pytest.mark.gpu

SHAPES = shape_cases()


@pytest.mark.parametrize("case", SHAPES, ids=[c[0] for c in SHAPES])
def test_shape_cases(case):
    name, V, T, target, _dtype, _kind = case
    dec = build(V)
    x = case_input(case)
    dev = torch.from_numpy(x).cuda()
    for fold in (None,) + (FOLDS if T <= 300 else ("mean",)):
        a = dec.align(x, tokens=target, confidence=fold)  # (a host array: staged)
        check_aligned(a, x, target, dec, fold, "%s %s host" % (name, fold))
        b = dec.align(dev, tokens=target, confidence=fold)  # (a device tensor: read in place)
        check_aligned(b, x, target, dec, fold, "%s %s device" % (name, fold))
        assert same(a, b)


@pytest.mark.parametrize("V", [29, 131, 1024])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32, torch.float64])
def test_device_tensors(dtype, V):
    """Rows of every dtype, at vocabularies whose rows are and are not 16-byte aligned (131 labels: row_lse's element loads for
    rows off a 16-byte boundary and for the labels left over after the last whole vector); an odd first row through a view that starts one label in."""
    dec = build(V)
    rng = np.random.default_rng(V)
    xs, targets = [], []
    for T, L in ((37, 9), (64, 30), (5, 2)):
        xs.append(torch.from_numpy(random_logits(rng, T, V)).to(dtype).cuda())
        targets.append(random_target(rng, L, V, doubled=1))
    flat = torch.from_numpy(random_logits(rng, 20 * V + 1, 1)[:, 0]).to(dtype).cuda()
    xs.append(flat[1:].view(20, V))  # (contiguous, but its base is one element past an aligned address)
    targets.append(random_target(rng, 6, V))
    got = dec.align_batch(xs, tokens=targets, confidence="mean")
    for u, (x, target) in enumerate(zip(xs, targets)):
        host = x.double().cpu().numpy()
        # (the widened values are exact; the tolerance class of the confidences is that of the input dtype)
        ref = host if dtype == torch.float64 else host.astype(np.float32)
        check_aligned(got[u], ref, target, dec, "mean", "%s V=%d utt %d" % (dtype, V, u))


def test_ragged_batch_list_and_tensor():
    dec = build(29)
    xs, targets = ragged_batch()
    dev = [torch.from_numpy(x).cuda() for x in xs]
    batch = dec.align_batch(dev, tokens=targets, confidence="mean")
    for u, (x, target) in enumerate(zip(xs, targets)):
        check_aligned(batch[u], x, target, dec, "mean", "utt %d" % u)
        assert same(batch[u], dec.align(dev[u], tokens=target, confidence="mean")), u
    T = max(len(x) for x in xs)
    pad = np.zeros((len(xs), T, 29))
    for u, x in enumerate(xs):
        pad[u, : len(x)] = x
    cube = dec.align_batch(torch.from_numpy(pad).cuda(), tokens=targets, confidence="mean")
    for u, target in enumerate(targets):
        check_aligned(cube[u], pad[u], target, dec, "mean", "padded %d" % u)
        assert same(cube[u], dec.align(pad[u], tokens=target, confidence="mean")), u


def test_tiny_budget_takes_several_launches():
    dec = build(29)
    xs, targets = ragged_batch(seed=11)
    whole = dec.align_batch(xs, tokens=targets, confidence="max")
    assert dec.last_align_launches == 1
    biggest = max(len(x) * ((2 * len(t) + 1 + 3) // 4) for x, t in zip(xs, targets))
    split = dec.align_batch(xs, tokens=targets, confidence="max", _bp_budget=biggest)
    assert dec.last_align_launches > 3
    assert all(same(a, b) for a, b in zip(whole, split))


def test_paths_equal_the_simulator(monkeypatch):
    """Random float64 logits have no exact score ties: the HIP path's frames are the simulator's, label for label."""
    from pyctcdecode_amd import _binding as B
    from tests.sim.build_sim import build as build_sim

    cases = [c for c in SHAPES if c[5] == "logits" and c[4] == np.float64 and c[2] <= 300]
    xs, targets = ragged_batch(seed=21)
    dec = build(29)
    hip_batch = dec.align_batch(xs, tokens=targets, confidence="mean")
    hip_cases = [build(c[1]).align(case_input(c), tokens=c[3], confidence="mean") for c in cases]
    monkeypatch.setattr(B, "_LIB", B.Library(build_sim()))
    sim = build(29)
    sim_batch = sim.align_batch(xs, tokens=targets, confidence="mean")
    for u, (a, b) in enumerate(zip(hip_batch, sim_batch)):
        assert np.array_equal(a.path, b.path) and a.token_frames == b.token_frames and a.text_frames == b.text_frames, u
        assert abs(a.score - b.score) <= 1e-9 and all(abs(p - q) <= 1e-9 for p, q in zip(a.token_logp, b.token_logp)), u
    for c, a in zip(cases, hip_cases):
        b = build(c[1]).align(case_input(c), tokens=c[3], confidence="mean")
        assert np.array_equal(a.path, b.path) and a.token_frames == b.token_frames, c[0]
        assert abs(a.score - b.score) <= 1e-9, c[0]


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_golden_words_overlap(name):
    from pyctcdecode_amd import build_ctcdecoder

    case, x, text, frames = golden_case(name)
    dec = build_ctcdecoder(case["labels"])
    a = dec.align(x, text, confidence="mean")
    labels = dec._alphabet.labels
    check_aligned(a, x, [labels.index(c) for c in " ".join(text.split())], dec, "mean", name)
    assert overlaps(a.text_frames, frames), (a.text_frames, frames)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32, torch.float64])
def test_result_does_not_depend_on_where_the_rows_lie(dtype):
    """Padding rows of zeros tie every path through them, and such ties are settled by the last bit of a row's
    log-sum-exp: the same matrix at a 16-byte boundary, one element past it and staged from the host gives the same bits."""
    V, T = 29, 41
    dec = build(V)
    rng = np.random.default_rng(17)
    target = random_target(rng, 9, V, doubled=1)
    x = torch.from_numpy(random_logits(rng, T, V)).to(dtype)
    x[23:] = 0
    flat = torch.zeros(T * V + 1, dtype=dtype).cuda()
    flat[1:] = x.reshape(-1).cuda()
    a = dec.align(x.cuda(), tokens=target, confidence="mean")
    b = dec.align(flat[1:].view(T, V), tokens=target, confidence="mean")
    c = dec.align(x.numpy(), tokens=target, confidence="mean")
    assert same(a, b) and same(a, c)
