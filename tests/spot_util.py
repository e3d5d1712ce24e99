"""Phrase spotting (spot / spot_batch; DESIGN.md "Phrase spotting") for the CPU and GPU tests: the recursion in numpy over
tests/token_logp_util.lp_matrix, written from the definition with np.logaddexp and not from csrc/ctc_align.h, the enumeration
of every frame-level path of a tiny input, the cases, and the comparison every PhraseSpot goes through."""
import itertools
import math

import numpy as np

from tests.align_util import SCORE_TOL, feasible, random_logits, random_target
from tests.find_util import pick_np
from tests.token_logp_util import lp_matrix

HALF_MARGIN = 1e-6  # end_start is compared where the reference's mean start lies farther than this from a half-integer


def log1mexp(x):
    with np.errstate(divide="ignore"):
        return np.where(x > -math.log(2.0), np.log(-np.expm1(x)), np.log1p(-np.exp(x)))


def spot_np(lp, phrase, blank):
    """(end_logp [T], mean_start [T], count) of the definition: a[s] the log-mass and m[s] the mass-weighted mean start frame
    of interior state s, a fresh start in state 1 weighted with 1 - p(t - 1, y[0]), an end weighted with 1 - p(t + 1, y[L-1])."""
    T, L = lp.shape[0], len(phrase)
    ext = np.full(2 * L + 1, blank, dtype=np.int64)
    ext[1::2] = phrase
    S = len(ext)
    can_skip = np.zeros(S, dtype=bool)
    can_skip[3::2] = ext[3::2] != ext[1:-2:2]
    interior = np.zeros(S, dtype=bool)
    interior[1:S - 1] = True
    a, m = np.full(S, -np.inf), np.zeros(S)
    end_logp, mean_start = np.full(T, -np.inf), np.zeros(T)
    for t in range(T):
        fresh = np.full(S, -np.inf)
        fresh[1] = 0.0 if t == 0 else log1mexp(lp[t - 1, phrase[0]])
        cand = np.stack([a, np.concatenate(([-np.inf], a[:-1])), np.where(can_skip, np.concatenate(([-np.inf, -np.inf], a[:-2])), -np.inf),
                         fresh])
        begun = np.stack([m, np.concatenate(([0.0], m[:-1])), np.concatenate(([0.0, 0.0], m[:-2])), np.full(S, float(t))])
        tot = np.logaddexp.reduce(cand, axis=0)
        with np.errstate(invalid="ignore"):
            w = np.where(np.isfinite(cand), np.exp(cand - tot), 0.0)
        a = np.where(interior, tot + lp[t, ext], -np.inf)
        m = np.where(np.isfinite(a), (w * begun).sum(axis=0), 0.0)
        right = 0.0 if t == T - 1 else log1mexp(lp[t + 1, phrase[-1]])
        end_logp[t], mean_start[t] = a[S - 2] + right, m[S - 2]
    return end_logp, mean_start, float(np.exp(end_logp).sum())


def enumerate_occurrences(x, blank, max_labels=3):
    """{phrase: [T] summed probability of the paths, of all V^T, with a maximal occurrence of it ending on frame t}"""
    p = np.exp(lp_matrix(x))
    T, V = p.shape
    table = {}
    for pi in itertools.product(range(V), repeat=T):
        weight = float(np.prod(p[np.arange(T), pi]))
        seen = set()
        for t in range(T):
            if pi[t] == blank or (t + 1 < T and pi[t + 1] == pi[t]):
                continue
            for s in range(t + 1):
                if pi[s] == blank or (s > 0 and pi[s - 1] == pi[s]):
                    continue
                y = tuple(c for k, c in enumerate(pi[s:t + 1]) if c != blank and (k == 0 or pi[s + k - 1] != c))
                if len(y) <= max_labels:
                    assert (y, t) not in seen  # (for a fixed end frame the events of different starts are disjoint)
                    seen.add((y, t))
                    table.setdefault(y, np.zeros(T))[t] += weight
    return table


def length_cases():
    """(L, T, phrase, x): lengths at the wave kernel's lane and wave edges and at the group kernel's two sizes; frames that just
    fit, one to spare, about 300. Seeds that keep every reference mean HALF_MARGIN off a half-integer (test_spot.py asserts it)."""
    cases = []
    for L in (1, 2, 31, 32, 63, 64, 127, 128, 129, 511, 512):
        rng = np.random.default_rng(4000 + L)
        phrase = random_target(rng, L, 29, doubled=min(2, L // 2))
        need = L + sum(1 for a, b in zip(phrase, phrase[1:]) if a == b)
        for T in sorted({need, need + 1, max(300, need + 7)}):
            x = random_logits(rng, T, 29)
            t = (T - need) // 2  # (the phrase once, +10 along its tightest path: a count that does not underflow)
            for k, c in enumerate(phrase):
                t += k > 0 and phrase[k - 1] == c
                x[t, c] += 10.0
                t += 1
            cases.append((L, T, phrase, x))
    return cases


def same(a, b):
    """Two PhraseSpot results float for float, window for window, and frame for frame of their traces."""
    if (a.text, a.tokens, a.hits, a.count) != (b.text, b.tokens, b.hits, b.count) or (a.end_logp is None) != (b.end_logp is None):
        return False
    return a.end_logp is None or (np.array_equal(a.end_logp, b.end_logp) and np.array_equal(a.end_start, b.end_start))


def check_spot(got, x, phrase, blank, max_hits=1, min_logp=-np.inf, what=""):
    """One traced PhraseSpot against spot_np on the matrix as given: end_logp within SCORE_TOL and -inf exactly, count within
    1e-9 relative, end_start wherever the reference's mean is HALF_MARGIN off a half-integer (returned), the hits equal to
    the selection run on the reference's trace."""
    want_logp, want_mean, want_count = spot_np(lp_matrix(np.asarray(x)), list(phrase), blank)
    T = len(want_logp)
    assert got.tokens == list(phrase) and got.end_logp.dtype == np.float64 and got.end_start.dtype == np.int32, what
    assert got.end_logp.shape == (T,) and got.end_start.shape == (T,), what
    fin = np.isfinite(want_logp)
    assert np.array_equal(np.isfinite(got.end_logp), fin) and np.all(got.end_logp[~fin] == -np.inf), what
    assert np.all(got.end_start[~fin] == -1), what
    gap = float(np.max(np.abs(got.end_logp[fin] - want_logp[fin]))) if fin.any() else 0.0
    print("%s: worst gap to numpy %.2e over %d end frames, count %.12g against %.12g" % (what, gap, int(fin.sum()), got.count, want_count))
    assert gap <= SCORE_TOL, (what, gap)
    assert abs(got.count - want_count) <= 1e-9 * want_count, (what, got.count, want_count)
    sure = fin & (np.abs(want_mean - np.floor(want_mean) - 0.5) > HALF_MARGIN)
    assert np.array_equal(got.end_start[sure], np.rint(want_mean[sure]).astype(np.int32)), what
    # the selection, restated over the reference trace (its scores lie within SCORE_TOL: the same frames unless two tie that closely)
    want_start = np.where(sure, np.rint(want_mean), got.end_start).astype(np.int32)
    want_hits = pick_np(want_logp, want_start, max_hits, min_logp)
    assert [(h.start, h.end) for h in got.hits] == [(s, e) for s, e, _ in want_hits], (what, got.hits, want_hits)
    for h, (_, e, v) in zip(got.hits, want_hits):
        assert abs(h.logp - v) <= SCORE_TOL and h.logp == got.end_logp[e - 1] and h.start == got.end_start[e - 1], (what, h)
        assert h.frames == h.end - h.start and h.prob == math.exp(h.logp), (what, h)
    return sure

