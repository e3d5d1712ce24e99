"""GPU (-m gpu): transcript likelihood of long transcripts (score_long / score_long_batch) on the HIP build -- row_lse and
ctc_forward_tile of csrc/ctc_align_hip.hip. The tests of tests/test_score_long.py from host arrays and from device tensors:
every shape case equal to score on the same device bit for bit at every tile shape, hypotheses above 2047 labels against the
numpy recursion, device tensors of every dtype, budgets, and the HIP build against the simulator."""
import pytest
import torch

from tests.score_long_util import (ABOVE, ABOVE_TILE, SHAPES, above_input, build, case_input, check_above, check_equals_score,
                                   check_hypotheses_batch, hypotheses_batch)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", SHAPES, ids=[c[0] for c in SHAPES])
def test_equals_score_at_every_tile_shape(case):
    name, V, T, target, _dtype, _kind = case
    x = case_input(case)
    skipped = check_equals_score(build(V), x, target, name, T, inputs=[x, torch.from_numpy(x).cuda()])
    if name.endswith("_T300"):
        assert skipped, name


@pytest.mark.parametrize("case", ABOVE, ids=[c[0] for c in ABOVE])
def test_above_2047_labels_against_numpy(case):
    """Largest |logp - numpy| seen on the device: 7.3e-12 (L4100_T4400: logp -10890.5, bound 8.5e-8; V29_L3000_T9000_f32:
    logp -33989.7, bound 5.4e-7), the simulator's figures; the asserted bound is 8 T eps |logp| (score_long_util.check_above)."""
    _target, x = above_input(case)
    check_above(build(case[1]), case, inputs=[x, torch.from_numpy(x).cuda()])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32, torch.float64])
def test_device_tensors(dtype):
    """Rows of every dtype read in place, several hypotheses per utterance: equal with == to single calls, to the staged host
    copy and to score_batch where it accepts the hypothesis."""
    xs, hyps, dead = hypotheses_batch()
    xs = [torch.from_numpy(x).to(dtype).cuda() for x in xs]
    hosts = None if dtype == torch.bfloat16 else [x.cpu().numpy() for x in xs]  # (numpy has no bfloat16 to stage from)
    check_hypotheses_batch(build(29), xs, hyps, dead, hosts)


def test_small_budget_takes_several_launch_groups():
    dec = build(29)
    xs, hyps, _dead = hypotheses_batch()
    xs = [torch.from_numpy(x).cuda() for x in xs]
    whole = dec.score_long_batch(xs, tokens=hyps)
    smallest = dec._score_long_plan(2500, 2100, 1, 0, 0)[4]
    split = dec.score_long_batch(xs, tokens=hyps, _budget=smallest)
    assert dec.last_score_long_groups > 1
    assert [[h.logp for h in cur] for cur in split] == [[h.logp for h in cur] for cur in whole]
    with pytest.raises(ValueError, match=r"utterance 0, hypothesis 0 .* %d bytes" % smallest):
        dec.score_long_batch(xs, tokens=hyps, _budget=smallest - 1)


def test_equals_the_simulator(monkeypatch):
    """The same tiles, the same operands in the same order, and the device's exp / log round as the host's on this input:
    the scores are equal with == (measured: both -4867.4519056334339)."""
    from pyctcdecode_amd import _binding as B
    from tests.sim.build_sim import build as build_sim

    case = ABOVE[1]
    target, x = above_input(case)
    hip = build(case[1]).score_long_batch([x], tokens=[[target]], _tile_groups=ABOVE_TILE[0], _tile_frames=ABOVE_TILE[1])[0][0].logp
    monkeypatch.setattr(B, "_LIB", B.Library(build_sim()))
    sim = build(case[1]).score_long_batch([x], tokens=[[target]], _tile_groups=ABOVE_TILE[0], _tile_frames=ABOVE_TILE[1])[0][0].logp
    assert hip == sim, (hip, sim)
