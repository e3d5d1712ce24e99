"""Alignment with gaps of long transcripts (BeamSearchDecoderCTC.align_gaps_long / align_gaps_long_batch; DESIGN.md "Alignment
with gaps, long transcripts"), shared by the CPU and GPU tests. Every function takes `inputs`: what turns a host array into
the forms the calls are given (the GPU tests add a device tensor); every form must give the same bits."""
import numpy as np

from tests.align_gaps_util import (FOLDS, GAP, PATTERNS, SCORE_TOL, case_input, check_gapped, equals_plain, g_of, gap_cases,
                                   gaps_of_pattern, items_of, same_gapped, sum_in_order)
from tests.align_long_util import ABOVE, ABOVE_SEGMENT, above_input, build, mixed_batch, plan_of, segment_lengths
from tests.align_util import random_logits, random_target
from tests.token_logp_util import lp_matrix

CASES = gap_cases()
U = 2  # GAPS_LONG_BATCH of csrc/ctc_align.h: at 2048 * U + 1 labels a thread owns one group more than a batch holds
BATCH_PLUS_ONE = ("L%d_T%d" % (2048 * U + 1, 2048 * U + 101), 5, 2048 * U + 1, 2048 * U + 101, 0, np.float64)
GAPPED_ABOVE = [("L2048_T2298", 5, 2048, 2298, 20, np.float64), ("L2049_T2299", 5, 2049, 2299, 0, np.float64)]
GAPPED_RUNS = [(c, p) for c in GAPPED_ABOVE for p in ("both", "middle", "doubled") if p != "doubled" or c[4]]
HOST = (lambda x: x,)
THREADS = "CTCDEC_GAPS_LONG_THREADS"


def cuts_of(name, T):
    return [0, 7, 1000] if name.startswith(("L511", "L512")) else segment_lengths(name, T)


def run_equals_align_gaps(case, monkeypatch, inputs=HOST):
    """align_gaps_long == align_gaps under every pattern, fold and cut, with the plan that was forced; the cases around the
    switch of workgroup size under both sizes."""
    name, V, T, target, _dtype, _kind = case
    dec = build(V)
    x = case_input(case)
    for pattern in PATTERNS:
        gaps = gaps_of_pattern(pattern, target)
        if gaps is None:
            continue
        items = items_of(target, gaps)
        for fold in (None,) + FOLDS:
            want = dec.align_gaps(x, tokens=items, confidence=fold)
            for K in cuts_of(name, T):
                for xin in (f(x) for f in inputs):
                    got = dec.align_gaps_long_batch([xin], tokens=[items], confidence=fold, _segment_frames=K)[0]
                    assert same_gapped(got, want), (name, pattern, fold, K)
                    assert dec.last_align_gaps_long_plan == [plan_of(T, K)] and dec.last_align_gaps_long_launches == 1
        if name.startswith(("L511", "L512")):
            for threads in ("256", "1024"):
                monkeypatch.setenv(THREADS, threads)
                for K in (0, 7):
                    got = dec.align_gaps_long_batch([inputs[-1](x)], tokens=[items], confidence="mean", _segment_frames=K)[0]
                    assert same_gapped(got, dec.align_gaps(x, tokens=items, confidence="mean")), (name, pattern, threads, K)
            monkeypatch.delenv(THREADS)


def planted_ties():
    """The input of tests/test_align_gaps.py's tie-rule test: every label its row's maximum on three consecutive frames."""
    rng = np.random.default_rng(5)
    target, x, t, want = [7, 12, 12, 5], rng.standard_normal((44, 29)), 10, []
    for c in target:
        x[t:t + 3, c] += 30.0
        want.append((t, t + 3))
        x[t + 3, 0] += 30.0
        t += 4
    return x, target, want


def run_ties_across_a_boundary(K, inputs=HOST):
    dec = build(29)
    x, target, want = planted_ties()
    items = [GAP] + target + [GAP]
    for xin in (f(x) for f in inputs):
        a = dec.align_gaps_long_batch([xin], tokens=[items], confidence="mean", _segment_frames=K)[0]
        assert [f for _lab, f in a.token_frames] == want, (K, a.token_frames)
        assert same_gapped(a, dec.align_gaps(x, tokens=items, confidence="mean")), K


def whole_and_cut(dec, xin, items, fold=None):
    out = [dec.align_gaps_long_batch([xin], tokens=[items], confidence=fold, _segment_frames=K)[0] for K in (0, ABOVE_SEGMENT)]
    assert same_gapped(out[0], out[1])
    return out[0]


def run_gap_free_equals_align_long(case, inputs=HOST):
    target, x = above_input(case)
    dec = build(case[1])
    for xin in (f(x) for f in inputs):
        for K in (0, ABOVE_SEGMENT):
            got = dec.align_gaps_long_batch([xin], tokens=[target], confidence="mean", _segment_frames=K)[0]
            assert equals_plain(got, dec.align_long_batch([xin], tokens=[target], confidence="mean", _segment_frames=K)[0]), (case[0], K)


def run_gapped_above(case, pattern, inputs=HOST):
    """Above 2047 labels with gaps, against numpy: -> |score - numpy optimum|."""
    target, x = above_input(case)
    gaps = gaps_of_pattern(pattern, target)
    dec = build(case[1])
    plain = dec.align_long(x, tokens=target).score
    every = dec.align_gaps_long(x, tokens=items_of(target, [1] * (len(target) + 1))).score
    got = [whole_and_cut(dec, f(x), items_of(target, gaps)) for f in inputs]
    assert all(same_gapped(got[0], g) for g in got[1:])
    best = check_gapped(got[0], x, target, gaps, dec, None, "%s %s" % (case[0], pattern), plain, every)
    print("%s %s: |score - numpy optimum| = %.3e" % (case[0], pattern, abs(got[0].score - best)))
    return abs(got[0].score - best)


def run_batch_plus_one_with_gaps(inputs=HOST):
    target, x = above_input(BATCH_PLUS_ONE)
    dec = build(5)
    lp = lp_matrix(x)
    g = g_of(lp)
    for xin in (f(x) for f in inputs):
        a = whole_and_cut(dec, xin, items_of(target, [1] * (len(target) + 1)))
        assert a.score >= dec.align_long(xin, tokens=target).score
        along = sum_in_order(g[t] if c == GAP else lp[t, int(c)] for t, c in enumerate(a.path))
        assert abs(a.score - along) <= SCORE_TOL, (a.score, along)


def gapped_mixed_batch():
    """mixed_batch() of the long tests without its targets that have no label, gaps added by pattern: (xs, items, infeasible)"""
    xs, targets, bad = mixed_batch()
    keep = [u for u, t in enumerate(targets) if t]
    items = [items_of(targets[u], gaps_of_pattern(PATTERNS[1 + j % 4], targets[u])) for j, u in enumerate(keep)]
    return [xs[u] for u in keep], items, keep.index(bad)


def run_mixed_batch(inputs=HOST):
    dec = build(29)
    xs, items, bad = gapped_mixed_batch()
    for f in inputs:
        xin = [f(x) for x in xs]
        for K in (0, 7):
            batch = dec.align_gaps_long_batch(xin, tokens=items, confidence="mean", strict=False, _segment_frames=K)
            assert dec.last_align_gaps_long_plan == [plan_of(len(x), K) for u, x in enumerate(xs) if u != bad]
            assert dec.last_align_gaps_long_launches == 1 and batch[bad] is None
            for u in range(len(xs)):
                if u != bad:
                    assert same_gapped(batch[u], dec.align_gaps_long(xs[u], tokens=items[u], confidence="mean")), (K, u)
        xin, its = [x for u, x in enumerate(xin) if u != bad], [t for u, t in enumerate(items) if u != bad]
        split = dec.align_gaps_long_batch(xin, tokens=its, confidence="mean", _bp_budget=640000)
        assert dec.last_align_gaps_long_launches > 1 and (272, 9) in dec.last_align_gaps_long_plan
        assert all(same_gapped(a, b) for a, b in zip(split, [b for b in batch if b is not None]))
