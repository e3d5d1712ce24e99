"""GPU (-m gpu): alignment with gaps (align_gaps / align_gaps_batch) on the HIP build -- row_lse_max and ctc_viterbi_gaps of
csrc/ctc_align_hip.hip. The shape cases, patterns and planted inputs of tests/test_align_gaps.py from host arrays and from
device tensors, a gap-free target against the HIP align exactly (which pins row_lse_max's bits to row_lse's), device tensors
of every dtype read in place at vocabularies where row_lse_max's vector and element loads differ, probability tensors,
ragged batches through a list and a [B, T, V] tensor, a batch forced over a tiny budget into several launches, and paths
equal to the CPU simulator's on inputs without score ties."""
import numpy as np
import pytest
import torch

from tests.align_gaps_util import (GAP, PATTERNS, case_input, check_gapped, equals_plain, gap_cases, gaps_of_pattern, items_of,
                                   same_gapped)
from tests.align_util import random_logits, random_target
from tests.test_align import build
from tests.test_align_gaps import (gapped_batch, run_batch_equals_single_calls, run_planted_pair, run_planted_phrase,
                                   run_planted_ties, run_shape_case, run_tiny_budget)

pytestmark = pytest.mark.gpu

CASES = gap_cases()


def on_device(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_shape_cases(case):
    """Every case under every pattern from a host array (staged) and from a device tensor (read in place): each against numpy
    and against the HIP align where there is no gap, and the two equal field for field."""
    host = run_shape_case(case)
    dev = run_shape_case(case, on_device)
    assert host.keys() == dev.keys()
    for pattern in host:
        assert same_gapped(host[pattern], dev[pattern]), (case[0], pattern)


@pytest.mark.parametrize("V", [29, 131, 1024])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32, torch.float64])
def test_device_tensors(dtype, V):
    """Rows of every dtype, at vocabularies whose rows are and are not 16-byte aligned (131 labels: row_lse_max's element loads
    for rows off a 16-byte boundary and for the labels left over after the last whole vector); an odd first row through a view
    that starts one label in. Without gaps the result is the HIP align's, exactly."""
    dec = build(V)
    rng = np.random.default_rng(V)
    xs, targets = [], []
    for T, L in ((37, 9), (64, 30), (5, 2)):
        xs.append(torch.from_numpy(random_logits(rng, T, V)).to(dtype).cuda())
        targets.append(random_target(rng, L, V, doubled=1))
    flat = torch.from_numpy(random_logits(rng, 20 * V + 1, 1)[:, 0]).to(dtype).cuda()
    xs.append(flat[1:].view(20, V))  # (contiguous, but its base is one element past an aligned address)
    targets.append(random_target(rng, 6, V))
    plain = dec.align_batch(xs, tokens=targets, confidence="mean")
    none = dec.align_gaps_batch(xs, tokens=targets, confidence="mean")
    every = dec.align_gaps_batch(xs, tokens=[items_of(t, [1] * (len(t) + 1)) for t in targets])
    for pattern in ("both", "middle", "every"):
        all_gaps = [gaps_of_pattern(pattern, t) for t in targets]
        got = dec.align_gaps_batch(xs, tokens=[items_of(t, g) for t, g in zip(targets, all_gaps)], confidence="mean")
        for u, (x, target) in enumerate(zip(xs, targets)):
            host = x.double().cpu().numpy()
            # (the widened values are exact; the tolerance class of the confidences is that of the input dtype)
            ref = host if dtype == torch.float64 else host.astype(np.float32)
            check_gapped(got[u], ref, target, all_gaps[u], dec, "mean", "%s V=%d utt %d %s" % (dtype, V, u, pattern),
                         plain[u].score, every[u].score)
    for u in range(len(xs)):
        assert equals_plain(none[u], plain[u]), (dtype, V, u)


@pytest.mark.parametrize("V", [29, 131, 1024])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32, torch.float64])
def test_probability_tensors(dtype, V):
    """Probability-like utterances get no log-sum-exp: row_lse_max takes their maximum alone, through the same loads -- in one
    batch with a logit utterance, on and off a 16-byte boundary."""
    dec = build(V)
    rng = np.random.default_rng(V + 7)
    T = 33
    # (powers of two that sum to exactly 1 in every dtype and every order of summation: what is a probability row to numpy's
    # test is one to the device's)
    p = np.zeros((T, V))
    for t in range(T):
        cols = rng.choice(V, size=10, replace=False)
        p[t, cols] = [2.0 ** -k for k in range(1, 10)] + [2.0 ** -9]
    probs = torch.from_numpy(p).to(dtype).cuda()
    flat = torch.zeros(T * V + 1, dtype=dtype).cuda()
    flat[1:] = probs.reshape(-1)
    logits = torch.from_numpy(random_logits(rng, T, V)).to(dtype).cuda()
    targets = [random_target(rng, 8, V, doubled=1) for _ in range(3)]
    xs = [probs, logits, flat[1:].view(T, V)]
    plain = dec.align_batch(xs, tokens=targets, confidence="mean")
    none = dec.align_gaps_batch(xs, tokens=targets, confidence="mean")
    every = dec.align_gaps_batch(xs, tokens=[items_of(t, [1] * 9) for t in targets])
    all_gaps = [gaps_of_pattern("both", t) for t in targets]
    got = dec.align_gaps_batch(xs, tokens=[items_of(t, g) for t, g in zip(targets, all_gaps)], confidence="mean")
    for u, x in enumerate(xs):
        host = x.double().cpu().numpy()
        ref = host if dtype == torch.float64 else host.astype(np.float32)
        check_gapped(got[u], ref, targets[u], all_gaps[u], dec, "mean", "%s V=%d utt %d" % (dtype, V, u), plain[u].score,
                     every[u].score)
        assert equals_plain(none[u], plain[u]), (dtype, V, u)
        assert GAP in got[u].path.tolist()
    assert got[0].score == dec.align_gaps(probs, tokens=items_of(targets[0], all_gaps[0])).score


def test_ragged_batch_list_and_tensor():
    dec, xs, xin, _targets, _all_gaps, items, batch = run_batch_equals_single_calls(on_device)
    host = dec.align_gaps_batch(xs, tokens=items, confidence="mean")
    assert all(same_gapped(a, b) for a, b in zip(batch, host))
    T = max(len(x) for x in xs)
    pad = np.zeros((len(xs), T, 29))
    for u, x in enumerate(xs):
        pad[u, : len(x)] = x
    cube = dec.align_gaps_batch(on_device(pad), tokens=items, confidence="mean")
    for u in range(len(xs)):
        assert same_gapped(cube[u], dec.align_gaps(pad[u], tokens=items[u], confidence="mean")), u


def test_tiny_budget_takes_several_launches():
    run_tiny_budget()
    run_tiny_budget(on_device)


def test_planted_phrase_is_found_where_it_lies():
    run_planted_phrase()
    run_planted_phrase(on_device)


def test_planted_pair_with_a_gap_between():
    run_planted_pair()
    run_planted_pair(on_device)


def test_tie_rule_gives_a_label_all_of_its_frames():
    run_planted_ties()
    run_planted_ties(on_device)


def test_paths_equal_the_simulator(monkeypatch):
    """Random float64 logits have no exact score ties: the HIP path's frames and gaps are the simulator's."""
    from pyctcdecode_amd import _binding as B
    from tests.sim.build_sim import build as build_sim

    cases = [c for c in CASES if c[5] == "logits" and c[4] == np.float64 and c[2] <= 300]
    xs, targets, all_gaps = gapped_batch(seed=21)
    items = [items_of(t, g) for t, g in zip(targets, all_gaps)]

    def run_cases():
        out = []
        for c in cases:
            dec = build(c[1])
            x = case_input(c)
            for pattern in PATTERNS:
                gaps = gaps_of_pattern(pattern, c[3])
                if gaps is not None:
                    out.append(("%s %s" % (c[0], pattern), dec.align_gaps(x, tokens=items_of(c[3], gaps), confidence="mean")))
        return out

    hip_batch = build(29).align_gaps_batch(xs, tokens=items, confidence="mean")
    hip_cases = run_cases()
    monkeypatch.setattr(B, "_LIB", B.Library(build_sim()))
    sim_batch = build(29).align_gaps_batch(xs, tokens=items, confidence="mean")
    sim_cases = run_cases()
    pairs = [("utt %d" % u, a, b) for u, (a, b) in enumerate(zip(hip_batch, sim_batch))]
    pairs += [(name, a, b) for (name, a), (_n, b) in zip(hip_cases, sim_cases)]
    assert len(pairs) > 40
    for name, a, b in pairs:
        assert np.array_equal(a.path, b.path) and a.token_frames == b.token_frames and a.text_frames == b.text_frames, name
        assert a.gaps == b.gaps and a.text == b.text, name
        assert abs(a.score - b.score) <= 1e-9 and all(abs(p - q) <= 1e-9 for p, q in zip(a.token_logp, b.token_logp)), name
        assert all(abs(p - q) <= 1e-9 for p, q in zip(a.gap_logp, b.gap_logp)), name


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32, torch.float64])
def test_result_does_not_depend_on_where_the_rows_lie(dtype):
    """Padding rows of zeros tie every path through them -- a gap's g(t) with every label's emission there --, and such ties
    are settled by the last bit of a row's log-sum-exp and maximum: the same matrix at a 16-byte boundary, one element past it
    and staged from the host gives the same bits, with a leading and a trailing gap."""
    V, T = 29, 41
    dec = build(V)
    rng = np.random.default_rng(17)
    target = random_target(rng, 9, V, doubled=1)
    items = [GAP] + target + [GAP]
    x = torch.from_numpy(random_logits(rng, T, V)).to(dtype)
    x[23:] = 0
    flat = torch.zeros(T * V + 1, dtype=dtype).cuda()
    flat[1:] = x.reshape(-1).cuda()
    a = dec.align_gaps(x.cuda(), tokens=items, confidence="mean")
    b = dec.align_gaps(flat[1:].view(T, V), tokens=items, confidence="mean")
    c = dec.align_gaps(x.numpy(), tokens=items, confidence="mean")
    assert same_gapped(a, b) and same_gapped(a, c)
    host = x.double().numpy()
    check_gapped(a, host if dtype == torch.float64 else host.astype(np.float32), target, [1] + [0] * 8 + [1], dec, "mean", str(dtype),
                 dec.align(x.cuda(), tokens=target).score)
