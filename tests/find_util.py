"""Phrase search (BeamSearchDecoderCTC.find / find_batch; DESIGN.md "Phrase search"), shared by the CPU and GPU tests: the
recursion with a free start and a free end and the selection of its hits in numpy over the clipped log-softmax of
tests/token_logp_util.lp_matrix -- written from the definition, not from csrc/ctc_align.h --, the maker of inputs with planted
occurrences, and the properties every PhraseSearch goes through. Windows are compared exactly with the yardstick's only on
planted inputs, where the margin is nats, not rounding: on random inputs two near-equal windows may both be right."""
import math

import numpy as np

from tests.align_util import SCORE_TOL, case_input, feasible, random_logits, random_target, shape_cases, viterbi_np
from tests.token_logp_util import lp_matrix

WAVE_MAX_LABELS = 127  # FIND_WAVE_MAX_LABELS of csrc/ctc_align.h
MAX_HITS = 64          # FIND_MAX_HITS


def find_np(lp, phrase, blank):
    """(end_logp [T] float64, end_start [T] int32): per frame t the score and the first frame of the best occurrence of
    `phrase` whose last label sits on t, -inf / -1 where none ends. States as in viterbi_np, but only 1 .. S - 2 exist; a
    state takes the best of stay, step (s >= 2), skip (s >= 3, a label that differs from the one before) and, for s = 1, a
    fresh start of 0.0 begun at t -- the earlier on equal scores -- plus lp[t, label of s]."""
    T, L = lp.shape[0], len(phrase)
    assert L >= 1
    ext = np.full(2 * L + 1, blank, dtype=np.int64)
    ext[1::2] = phrase
    S = len(ext)
    can_skip = np.zeros(S, dtype=bool)
    can_skip[3::2] = ext[3::2] != ext[1:-2:2]
    interior = np.zeros(S, dtype=bool)
    interior[1:S - 1] = True
    cols = np.arange(S)
    d, st = np.full(S, -np.inf), np.full(S, -1, dtype=np.int64)
    end_logp, end_start = np.full(T, -np.inf), np.full(T, -1, dtype=np.int32)
    for t in range(T):
        fresh = np.full(S, -np.inf)
        fresh[1] = 0.0
        cand = np.stack([d, np.concatenate(([-np.inf], d[:-1])), np.where(can_skip, np.concatenate(([-np.inf, -np.inf], d[:-2])), -np.inf),
                         fresh])
        begun = np.stack([st, np.concatenate(([-1], st[:-1])), np.concatenate(([-1, -1], st[:-2])), np.full(S, t, dtype=np.int64)])
        k = np.argmax(cand, axis=0)  # (the first of equal maxima: stay, step, skip, fresh)
        d = np.where(interior, cand[k, cols] + lp[t, ext], -np.inf)
        st = np.where(np.isfinite(d), begun[k, cols], -1)
        end_logp[t], end_start[t] = d[S - 2], st[S - 2]
    return end_logp, end_start


def overlaps(start, t, taken):
    """Does the window of frames [start, t] share a frame with one of the (start, end) windows taken?"""
    return any(start < e and s <= t for s, e, *_ in taken)


def pick_np(end_logp, end_start, max_hits, min_logp=-np.inf):
    """The hits [(start, end, logp)], best first: until max_hits are taken, the end frame with the largest finite
    end_logp >= min_logp whose window shares no frame with a window taken before, the smallest on a tie."""
    taken = []
    while len(taken) < max_hits:
        best = None
        for t in range(len(end_logp)):
            v = end_logp[t]
            if np.isfinite(v) and v >= min_logp and (best is None or v > end_logp[best]) and not overlaps(int(end_start[t]), t, taken):
                best = t
        if best is None:
            break
        taken.append((int(end_start[best]), best + 1, float(end_logp[best])))
    return taken


def yardstick(x, phrase, blank, max_hits=1, min_logp=-np.inf):
    """(hits, end_logp, end_start) of the definition for the matrix as given."""
    end_logp, end_start = find_np(lp_matrix(np.asarray(x)), list(phrase), blank)
    return pick_np(end_logp, end_start, max_hits, min_logp), end_logp, end_start


def planted_input(rng, T, V, phrase, blank, starts, dtype=np.float64):
    """(x, windows): unit-normal logits [T, V] in which `phrase` is planted at each frame of `starts`: +30 on a label's frame,
    +30 on the blank in the frame after it, so that an occurrence is the window [start, start + 2 L - 1)."""
    x = rng.standard_normal((T, V))
    windows = []
    for s0 in starts:
        assert s0 + 2 * len(phrase) <= T
        for k, c in enumerate(phrase):
            x[s0 + 2 * k, c] += 30.0
            x[s0 + 2 * k + 1, blank] += 30.0
        windows.append((s0, s0 + 2 * len(phrase) - 1))
    return x.astype(dtype), windows


def windows_of(found):
    return [(h.start, h.end) for h in found.hits]


def check_found(found, x, phrase, blank, max_hits=1, min_logp=-np.inf, what="", ref=None):
    """Every property of one PhraseSearch against numpy. `ref`: (end_logp, end_start) of find_np, where the caller has it.
    Returns them."""
    lp = lp_matrix(np.asarray(x))
    T = lp.shape[0]
    want_logp, want_start = ref if ref is not None else find_np(lp, list(phrase), blank)
    hits = found.hits
    assert found.tokens == list(phrase) and len(hits) <= max_hits, (what, len(hits))
    traced = found.end_logp is not None
    if traced:
        assert found.end_logp.dtype == np.float64 and found.end_logp.shape == (T,), what
        assert found.end_start.dtype == np.int32 and found.end_start.shape == (T,), what
        fin = np.isfinite(want_logp)
        assert np.array_equal(np.isfinite(found.end_logp), fin), what
        assert np.all(found.end_logp[~fin] == -np.inf) and np.all(found.end_start[~fin] == -1), what
        gap = float(np.max(np.abs(found.end_logp[fin] - want_logp[fin]))) if fin.any() else 0.0
        print("%s: trace, worst gap to numpy %.2e over %d end frames" % (what, gap, int(fin.sum())))
        assert gap <= SCORE_TOL, (what, gap)
        assert np.all((found.end_start[fin] >= 0) & (found.end_start[fin] <= np.flatnonzero(fin))), what
    else:
        assert found.end_start is None
    for k, h in enumerate(hits):
        assert 0 <= h.start < h.end <= T and h.frames == h.end - h.start and h.mean_logp == h.logp / h.frames, (what, h)
        assert math.isfinite(h.logp) and h.logp >= min_logp, (what, h, min_logp)
        # (the window's best path may begin or end on a blank; it cannot beat the hit unless an end frame inside the window
        # scored higher and was dropped because its own best window overlaps an earlier hit -- none of the cases here)
        best, _ = viterbi_np(lp[h.start:h.end], list(phrase), blank)
        print("%s: hit %d [%d, %d) logp %.12f, numpy's end_logp %.12f, best path of the window %.12f"
              % (what, k, h.start, h.end, h.logp, want_logp[h.end - 1], best))
        assert abs(h.logp - want_logp[h.end - 1]) <= SCORE_TOL, (what, h, want_logp[h.end - 1])
        assert abs(h.logp - best) <= SCORE_TOL, (what, h, best)
        if traced:
            assert found.end_logp[h.end - 1] == h.logp and found.end_start[h.end - 1] == h.start, (what, h)
        if k:
            assert h.logp <= hits[k - 1].logp, (what, k, h.logp, hits[k - 1].logp)
        for g in hits[:k]:
            assert h.end <= g.start or g.end <= h.start, (what, h, g)
    # nothing better was left behind: the end frames that were still to be had (by the call's own windows where it returns
    # them, else numpy's) score no more than the last hit -- and there are none at all when fewer than max_hits were taken
    starts = found.end_start if traced else want_start
    taken = windows_of(found)
    chosen = {h.end - 1 for h in hits}
    floor = hits[-1].logp if len(hits) == max_hits else -np.inf
    for t in range(T):
        v = want_logp[t]
        if t in chosen or not np.isfinite(v) or v < min_logp + SCORE_TOL or overlaps(int(starts[t]), t, taken):
            continue
        assert len(hits) == max_hits and v <= floor + SCORE_TOL, (what, t, v, floor, len(hits))
    return want_logp, want_start


def neg_inf_case():
    """(x, phrase): float64 logits [25, 29] that hold -inf at labels of the phrase in some frames (and at the blank in one):
    the emissions there take the floor ln 1e-15, and every score stays finite."""
    rng = np.random.default_rng(77)
    phrase = random_target(rng, 5, 29, doubled=1)
    x = random_logits(rng, 25, 29)
    for t in range(0, 25, 3):
        x[t, phrase[(t // 3) % len(phrase)]] = -np.inf
    x[4, 0] = -np.inf
    return x, phrase


__all__ = ["SCORE_TOL", "WAVE_MAX_LABELS", "MAX_HITS", "find_np", "pick_np", "overlaps", "yardstick", "planted_input", "windows_of",
           "check_found", "neg_inf_case", "case_input", "feasible", "shape_cases", "random_logits", "random_target"]
