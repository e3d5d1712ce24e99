"""GPU (-m gpu): forced alignment of long transcripts (align_long / align_long_batch) on the HIP build -- row_lse and
ctc_viterbi_long of csrc/ctc_align_hip.hip. The tests of tests/test_align_long.py from host arrays and from device tensors:
every shape case equal to align on the same device bit for bit at every forced segment length, targets above 2047 labels
against the numpy Viterbi, device tensors of every dtype, mixed batches and budgets."""
import numpy as np
import pytest
import torch

from tests.align_long_util import (ABOVE, SHAPES, above_input, build, case_input, check_above, check_equals_align, crosses,
                                   mixed_batch, plan_of, same)
from tests.align_util import SCORE_TOL, check_aligned, random_logits, random_target

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", SHAPES, ids=[c[0] for c in SHAPES])
def test_equals_align_at_every_segment_length(case):
    name, V, T, target, _dtype, _kind = case
    dec = build(V)
    x = case_input(case)
    at7 = check_equals_align(dec, x, target, name, T, inputs=[x, torch.from_numpy(x).cuda()])
    if name.endswith("_T300"):
        assert crosses(at7, 7), name


@pytest.mark.parametrize("case", ABOVE, ids=[c[0] for c in ABOVE])
def test_above_2047_labels_against_numpy(case):
    """Largest |score - numpy optimum| seen: 0 in all four cases, under the float64 SCORE_TOL = 1e-9"""
    _target, x = above_input(case)
    assert check_above(build(case[1]), case, inputs=[x, torch.from_numpy(x).cuda()]) <= SCORE_TOL


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32, torch.float64])
def test_device_tensors(dtype):
    """Rows of every dtype read in place, one batch: a target above 2047 labels, two below, whole and in segments; equal to the
    staged host copy with ==, to align where align accepts the target, and right against numpy."""
    V = 29
    dec = build(V)
    rng = np.random.default_rng(31)
    xs, targets = [], []
    for T, L, doubled in ((2500, 2100, 3), (300, 129, 4), (37, 9, 1)):
        xs.append(torch.from_numpy(random_logits(rng, T, V)).to(dtype).cuda())
        targets.append(random_target(rng, L, V, doubled=doubled))
    hosts = [x.double().cpu().numpy() if dtype == torch.bfloat16 else x.cpu().numpy() for x in xs]
    whole = dec.align_long_batch(xs, tokens=targets, confidence="mean")
    assert dec.last_align_long_plan == [plan_of(len(x), 0) for x in xs]
    cut = dec.align_long_batch(xs, tokens=targets, confidence="mean", _segment_frames=7)
    assert dec.last_align_long_plan == [plan_of(len(x), 7) for x in xs]
    assert all(same(a, b) for a, b in zip(whole, cut))
    for u, (x, host, target) in enumerate(zip(xs, hosts, targets)):
        if dtype != torch.bfloat16:  # (numpy has no bfloat16 to stage from)
            assert same(whole[u], dec.align_long_batch([host], tokens=[target], confidence="mean", _segment_frames=7)[0]), u
        if len(target) <= 2047:
            assert same(whole[u], dec.align(x, tokens=target, confidence="mean")), u
        # (the widened values are exact; the tolerance class of the confidences is that of the input dtype)
        ref = x.double().cpu().numpy()
        check_aligned(whole[u], ref if dtype == torch.float64 else ref.astype(np.float32), target, dec, "mean", "%s utt %d" % (dtype, u))


def test_mixed_batch_equals_single_calls():
    dec = build(29)
    xs, targets, bad = mixed_batch()
    dev = [torch.from_numpy(x).cuda() for x in xs]
    with pytest.raises(ValueError, match=r"\[%d\]" % bad):
        dec.align_long_batch(dev, tokens=targets)
    for K in (0, 7):
        batch = dec.align_long_batch(dev, tokens=targets, confidence="mean", strict=False, _segment_frames=K)
        assert dec.last_align_long_plan == [plan_of(len(x), K) for u, x in enumerate(xs) if u != bad]
        assert dec.last_align_long_launches == 1 and batch[bad] is None
        host = dec.align_long_batch(xs, tokens=targets, confidence="mean", strict=False, _segment_frames=K)
        for u, (x, target) in enumerate(zip(xs, targets)):
            if u == bad:
                continue
            assert same(batch[u], host[u]), (K, u)
            assert same(batch[u], dec.align_long_batch([dev[u]], tokens=[target], confidence="mean", _segment_frames=K)[0]), (K, u)
            if len(target) <= 2047:
                assert same(batch[u], dec.align(dev[u], tokens=target, confidence="mean")), (K, u)
            if len(x) and K == 0:
                check_aligned(batch[u], x, target, dec, "mean", "utt %d" % u)


def test_small_budget_takes_several_launches():
    dec = build(29)
    xs, targets, bad = mixed_batch()
    xs, targets = [x for u, x in enumerate(xs) if u != bad], [t for u, t in enumerate(targets) if u != bad]
    whole = dec.align_long_batch(xs, tokens=targets, confidence="max")
    assert dec.last_align_long_launches == 1
    split = dec.align_long_batch(xs, tokens=targets, confidence="max", _bp_budget=640000)
    assert dec.last_align_long_launches > 1 and dec.last_align_long_plan[3] == (272, 9)
    assert all(same(a, b) for a, b in zip(whole, split))
    smallest = dec._align_long_plan(2300, 2049, 1, 0)[2]
    with pytest.raises(ValueError, match=r"utterance 3 .* %d bytes" % smallest):
        dec.align_long_batch(xs, tokens=targets, _bp_budget=smallest - 1)
    assert all(same(a, b) for a, b in zip(whole, dec.align_long_batch(xs, tokens=targets, confidence="max")))


def test_paths_equal_the_simulator(monkeypatch):
    """Random float64 logits have no exact score ties: the HIP path's frames are the simulator's, label for label."""
    from pyctcdecode_amd import _binding as B
    from tests.sim.build_sim import build as build_sim

    case = ABOVE[1]
    target, x = above_input(case)
    hip = build(case[1]).align_long_batch([x], tokens=[target], confidence="mean", _segment_frames=97)[0]
    monkeypatch.setattr(B, "_LIB", B.Library(build_sim()))
    sim = build(case[1]).align_long_batch([x], tokens=[target], confidence="mean", _segment_frames=97)[0]
    assert np.array_equal(hip.path, sim.path) and hip.token_frames == sim.token_frames and hip.text_frames == sim.text_frames
    assert abs(hip.score - sim.score) <= 1e-9
