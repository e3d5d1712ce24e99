"""GPU (-m gpu): tiled forced alignment of long transcripts (align_long(tiled=True)) on the HIP build -- row_lse, ctc_viterbi_tile
and ctc_viterbi_cone of csrc/ctc_align_hip.hip. The tests of tests/test_align_tiled.py from host arrays and from device tensors:
every shape case equal to align on the same device bit for bit at every tile shape, targets above 2047 labels equal to
align_long and right against numpy, device tensors of every dtype, mixed batches and budgets, and the simulator's bits."""
import numpy as np
import pytest
import torch

from tests.align_long_util import SHAPES, above_input, build, case_input, crosses, mixed_batch, same
from tests.align_tiled_util import ABOVE, ABOVE_CUT, check_above, check_equals_align, check_mixed_batch, tiled
from tests.align_util import SCORE_TOL, random_logits, random_target

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", SHAPES, ids=[c[0] for c in SHAPES])
def test_equals_align_at_every_tile_shape(case):
    name, V, _T, target, _dtype, _kind = case
    dec = build(V)
    x = case_input(case)
    check_equals_align(dec, x, target, name, inputs=[x, torch.from_numpy(x).cuda()])
    if name.endswith("_T300"):
        assert crosses(tiled(dec, [x], [target], (3, 7, 1))[0], 7), name


@pytest.mark.parametrize("case", ABOVE, ids=[c[0] for c in ABOVE])
def test_above_2047_labels_equals_align_long_and_numpy(case):
    """Largest |score - numpy optimum| seen: 0 in all four cases, under the float64 SCORE_TOL = 1e-9"""
    _target, x = above_input(case)
    assert check_above(build(case[1]), case, inputs=[x, torch.from_numpy(x).cuda()]) <= SCORE_TOL


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32, torch.float64])
def test_device_tensors(dtype):
    """Rows of every dtype read in place, one batch -- a target above 2047 labels over three segments, two below: equal to
    align_long untiled on the same tensors and to the staged host copy"""
    V = 29
    dec = build(V)
    rng = np.random.default_rng(31)
    xs, targets = [], []
    for T, L, doubled in ((2500, 2100, 3), (300, 129, 4), (37, 9, 1)):
        xs.append(torch.from_numpy(random_logits(rng, T, V)).to(dtype).cuda())
        targets.append(random_target(rng, L, V, doubled=doubled))
    want = dec.align_long_batch(xs, tokens=targets, confidence="mean")
    for cut in ((0, 0, 0), ABOVE_CUT):
        got = tiled(dec, xs, targets, cut, confidence="mean")
        assert all(same(a, b) for a, b in zip(got, want)), cut
    if dtype != torch.bfloat16:  # (numpy has no bfloat16 to stage from)
        host = tiled(dec, [x.cpu().numpy() for x in xs], targets, confidence="mean")
        assert all(same(a, b) for a, b in zip(host, want))


def test_mixed_batch_and_budgets():
    dec = build(29)
    xs, targets, _bad = mixed_batch()
    most = check_mixed_batch(dec, [torch.from_numpy(x).cuda() for x in xs])
    with pytest.raises(ValueError, match=r"utterance 3 .*without tiled needs less.* %d bytes" % most):
        tiled(dec, xs, targets, strict=False, _bp_budget=most - 1)


def test_equals_the_simulator(monkeypatch):
    """Path, score and spans with ==. (No fold: a "mean" confidence of the two builds may differ in its last bit, as align's does --
    fold_token_logp is that call's code.)"""
    from pyctcdecode_amd import _binding as B
    from tests.sim.build_sim import build as build_sim

    case = ABOVE[1]
    target, x = above_input(case)
    hip = tiled(build(case[1]), [x], [target], ABOVE_CUT)[0]
    monkeypatch.setattr(B, "_LIB", B.Library(build_sim()))
    assert same(hip, tiled(build(case[1]), [x], [target], ABOVE_CUT)[0])
