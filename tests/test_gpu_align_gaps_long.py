"""GPU (-m gpu): alignment with gaps of long transcripts (align_gaps_long / align_gaps_long_batch) on the HIP build -- row_lse_max
and ctc_viterbi_gaps_long of csrc/ctc_align_hip.hip. The tests of tests/test_align_gaps_long.py from host arrays and from device
tensors, device tensors of every dtype, and paths equal to the CPU simulator's on an input with exact ties."""
import numpy as np
import pytest
import torch

from tests.align_gaps_long_util import (ABOVE, ABOVE_SEGMENT, BATCH_PLUS_ONE, CASES, GAPPED_RUNS, SCORE_TOL, above_input, build,
                                        gaps_of_pattern, items_of, random_logits, random_target, run_batch_plus_one_with_gaps,
                                        run_equals_align_gaps, run_gap_free_equals_align_long, run_gapped_above, run_mixed_batch,
                                        run_ties_across_a_boundary, same_gapped)

pytestmark = pytest.mark.gpu


def on_device(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


BOTH = (lambda x: x, on_device)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_equals_align_gaps_at_every_cut(case, monkeypatch):
    run_equals_align_gaps(case, monkeypatch, BOTH)


@pytest.mark.parametrize("K", [1, 2, 3])
def test_tie_rule_across_a_boundary(K):
    run_ties_across_a_boundary(K, BOTH)


@pytest.mark.parametrize("case", ABOVE[:2] + [BATCH_PLUS_ONE], ids=lambda c: c[0])
def test_gap_free_equals_align_long_above_2047_labels(case):
    run_gap_free_equals_align_long(case, BOTH)


@pytest.mark.parametrize("case,pattern", GAPPED_RUNS, ids=["%s_%s" % (c[0], p) for c, p in GAPPED_RUNS])
def test_gaps_above_2047_labels_against_numpy(case, pattern):
    """Largest |score - numpy optimum| seen: see DESIGN.md, "Alignment with gaps, long transcripts"."""
    assert run_gapped_above(case, pattern, BOTH) <= SCORE_TOL


def test_one_group_more_than_a_batch_with_every_slot_a_gap():
    run_batch_plus_one_with_gaps(BOTH)


def test_mixed_batch_and_budgets():
    run_mixed_batch(BOTH)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32, torch.float64])
def test_device_tensors(dtype):
    """One batch with a target above 2047 labels and two below, read in place: whole == cut at 7 == the staged host copy (where
    numpy has the dtype) == align_gaps where it accepts the target."""
    dec = build(29)
    rng = np.random.default_rng(31)
    xs, items = [], []
    for (T, L), pattern in zip(((2300, 2049), (300, 127), (40, 11)), ("both", "middle", "every")):
        xs.append(torch.from_numpy(random_logits(rng, T, 29)).to(dtype).cuda())
        target = random_target(rng, L, 29, doubled=1)
        items.append(items_of(target, gaps_of_pattern(pattern, target)))
    whole = dec.align_gaps_long_batch(xs, tokens=items, confidence="mean")
    cut = dec.align_gaps_long_batch(xs, tokens=items, confidence="mean", _segment_frames=7)
    small = dec.align_gaps_batch(xs[1:], tokens=items[1:], confidence="mean")
    assert all(same_gapped(a, b) for a, b in zip(whole, cut)) and all(same_gapped(a, b) for a, b in zip(whole[1:], small))
    if dtype != torch.bfloat16:
        host = dec.align_gaps_long_batch([x.cpu().numpy() for x in xs], tokens=items, confidence="mean", _segment_frames=7)
        assert all(same_gapped(a, b) for a, b in zip(whole, host))


def test_paths_equal_the_simulator(monkeypatch):
    """float32 logits rounded to few distinct values tie exactly, rows' maxima with target labels among them: the tie rules,
    not luck, decide the path -- and the HIP build decides as the simulator does."""
    from pyctcdecode_amd import _binding as B
    from tests.sim.build_sim import build as build_sim

    case = GAPPED_RUNS[0][0]
    target, x = above_input(case)
    x = np.round(x).astype(np.float32)
    items = items_of(target, gaps_of_pattern("both", target))
    hip = build(5).align_gaps_long_batch([x], tokens=[items], confidence="mean", _segment_frames=ABOVE_SEGMENT)[0]
    monkeypatch.setattr(B, "_LIB", B.Library(build_sim()))
    sim = build(5).align_gaps_long_batch([x], tokens=[items], confidence="mean", _segment_frames=ABOVE_SEGMENT)[0]
    assert np.array_equal(hip.path, sim.path) and hip.token_frames == sim.token_frames and hip.gaps == sim.gaps
    assert abs(hip.score - sim.score) <= SCORE_TOL and all(abs(p - q) <= SCORE_TOL for p, q in zip(hip.gap_logp, sim.gap_logp))
