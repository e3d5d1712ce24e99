"""Frame posteriors (BeamSearchDecoderCTC.posteriors / posteriors_batch; DESIGN.md "Frame posteriors"), shared by the CPU and
GPU tests: two yardsticks written from the definition, not from csrc/ctc_align.h -- a textbook float64 forward-backward in
numpy over the clipped log-softmax of tests/token_logp_util.lp_matrix, and, for tiny shapes, the posteriors by brute force
over every path --, the tolerances, and the checks every result goes through.

Tolerances, all from SCORE_TOL = 1e-9, the bound the float64 score tests hold up to T = 2100:
  GAMMA_TOL = 4 * SCORE_TOL absolute on every gamma: alpha, beta and logp each carry at most SCORE_TOL, and gamma <= 1, so
      exp turns the three log-domain errors into at most that much absolute error;
  T * GAMMA_TOL on occupancy against the yardstick (a sum of T gammas);
  SUM_RTOL = 1e-12 relative between occupancy / centre and the same sums taken in numpy over the RETURNED gamma: a sum of
      n <= 2100 non-negative terms in any order differs by at most n * 2^-53 = 2.4e-13 relative; two sums and a division stay
      under 1e-12."""
import itertools

import numpy as np

from tests.align_util import SCORE_TOL
from tests.token_logp_util import lp_matrix

GAMMA_TOL = 4 * SCORE_TOL
SUM_RTOL = 1e-12


def states_of(target, blank):
    ext = np.full(2 * len(target) + 1, blank, dtype=np.int64)
    ext[1::2] = target
    can_skip = np.zeros(len(ext), dtype=bool)
    can_skip[3::2] = ext[3::2] != ext[1:-2:2]
    return ext, can_skip


def fwdbwd_np(lp, target, blank):
    """(logp, gamma [T, 2 L + 1]) of `target` over the [T, V] float64 log-probabilities `lp`: gamma[t, s] is the share, among
    all alignments, of those that are in state s at frame t."""
    T = lp.shape[0]
    ext, can_skip = states_of(target, blank)
    S = len(ext)
    if T == 0:
        return 0.0, np.zeros((0, S))
    NEG = -np.inf
    with np.errstate(invalid="ignore"):  # (logaddexp(-inf, -inf) is -inf; numpy computes -inf - -inf on the way)
        alpha = np.full((T, S), NEG)
        alpha[0, 0] = lp[0, blank]
        if S > 1:
            alpha[0, 1] = lp[0, ext[1]]
        for t in range(1, T):
            padded = np.concatenate(([NEG, NEG], alpha[t - 1]))
            acc = np.logaddexp(alpha[t - 1], padded[1:S + 1])
            acc = np.logaddexp(acc, np.where(can_skip, padded[:S], NEG))
            alpha[t] = acc + lp[t, ext]
        logp = float(np.logaddexp(alpha[T - 1, S - 1], alpha[T - 1, S - 2]) if S > 1 else alpha[T - 1, 0])
        # beta[t, s]: everything after frame t, given state s at frame t
        beta = np.full((T, S), NEG)
        beta[T - 1, S - 1] = 0.0
        if S > 1:
            beta[T - 1, S - 2] = 0.0
        skip_from = np.concatenate((can_skip, [False, False]))[2:]  # state s may jump to s + 2
        for t in range(T - 2, -1, -1):
            nxt = np.concatenate((beta[t + 1] + lp[t + 1, ext], [NEG, NEG]))
            acc = np.logaddexp(nxt[:S], nxt[1:S + 1])
            beta[t] = np.logaddexp(acc, np.where(skip_from, nxt[2:S + 2], NEG))
        gamma = np.exp(alpha + beta - logp)
    return logp, gamma


def enumerate_np(lp, target, blank):
    """gamma by brute force, for tiny shapes: every sequence of T states is tried, those that are an alignment (start in
    state 0 or 1, end in S - 1 or S - 2, move by 0, 1 or -- onto a label that differs from the one before -- 2) are weighed
    by the product of their frames' probabilities, and each frame's states take their share of the total."""
    T = lp.shape[0]
    ext, can_skip = states_of(target, blank)
    S = len(ext)
    assert S ** T <= 200000, "enumerate_np is for tiny shapes"
    mass = np.zeros((T, S))
    total = 0.0
    for path in itertools.product(range(S), repeat=T):
        if path[0] > 1 or path[-1] < S - 2:
            continue
        ok = all(b - a in (0, 1) or (b - a == 2 and can_skip[b]) for a, b in zip(path, path[1:]))
        if not ok:
            continue
        w = float(np.exp(sum(lp[t, ext[s]] for t, s in enumerate(path))))
        total += w
        for t, s in enumerate(path):
            mass[t, s] += w
    return float(np.log(total)), mass / total


def window_mask(T, S):
    """[T, S] bool: the states an alignment can be in at each frame, S - 2 - 2 (T - 1 - t) <= s <= 2 t + 1."""
    t = np.arange(T)[:, None]
    s = np.arange(S)[None, :]
    return (s >= S - 2 - 2 * (T - 1 - t)) & (s <= 2 * t + 1)


def yardstick(x, target, blank):
    return fwdbwd_np(lp_matrix(np.asarray(x)), list(target), blank)


def check_posteriors(got, want, T, target, what):
    """Every property of one dense TranscriptPosteriors against the yardstick's (logp, gamma); prints the worst gaps."""
    want_logp, want_gamma = want
    L, S = len(target), 2 * len(target) + 1
    assert got.tokens == list(target)
    assert got.gamma.dtype == np.float64 and got.gamma.shape == (T, S), (what, got.gamma.shape)
    assert got.occupancy.dtype == np.float64 and got.occupancy.shape == (L,) and got.centre.shape == (L,)
    if T == 0:
        assert got.logp == 0.0 and got.logp_backward == 0.0
        return
    assert np.isfinite(got.gamma).all() and np.isfinite(got.occupancy).all() and np.isfinite(got.centre).all(), what
    gap_logp, gap_back = abs(got.logp - want_logp), abs(got.logp - got.logp_backward)
    gap_gamma = float(np.abs(got.gamma - want_gamma).max())
    gap_rows = float(np.abs(got.gamma.sum(axis=1) - 1.0).max())
    print("%s: logp %.12f, numpy %+.1e, backward %+.1e; gamma %.1e, rows %.1e" % (what, got.logp, gap_logp, gap_back, gap_gamma, gap_rows))
    assert gap_logp <= SCORE_TOL and gap_back <= SCORE_TOL, (what, got.logp, want_logp, got.logp_backward)
    assert gap_gamma <= GAMMA_TOL, (what, gap_gamma)
    assert gap_rows <= S * GAMMA_TOL, (what, gap_rows)
    assert (got.gamma[~window_mask(T, S)] == 0.0).all(), what
    assert np.array_equal(got.token_post, got.gamma[:, 1::2]) and np.array_equal(got.blank_post, got.gamma[:, 0::2].sum(axis=1))
    if L:
        occ = got.gamma[:, 1::2].sum(axis=0)
        cen = (np.arange(T)[:, None] * got.gamma[:, 1::2]).sum(axis=0) / occ
        gap_occ = float(np.abs(got.occupancy - want_gamma[:, 1::2].sum(axis=0)).max())
        rel_occ = float(np.abs(got.occupancy / occ - 1.0).max())
        with np.errstate(invalid="ignore"):
            rel_cen = float(np.nanmax(np.where(cen != 0.0, np.abs(got.centre - cen) / np.abs(cen), np.abs(got.centre))))
        print("%s: occupancy %.1e (relative to the returned gamma %.1e), centre %.1e" % (what, gap_occ, rel_occ, rel_cen))
        assert gap_occ <= T * GAMMA_TOL, (what, gap_occ)
        assert rel_occ <= SUM_RTOL, (what, rel_occ)
        assert (np.abs(got.centre - cen) <= SUM_RTOL * np.abs(cen)).all(), (what, rel_cen)
        assert (got.occupancy >= 1.0 - T * GAMMA_TOL).all(), (what, float(got.occupancy.min()))
    total = float(got.occupancy.sum() + got.blank_post.sum())
    assert abs(total - T) <= T * S * GAMMA_TOL, (what, total)


def same_bits(a, b, dense=True):
    """Two TranscriptPosteriors, float for float."""
    ok = (a.text == b.text and a.tokens == b.tokens and a.logp == b.logp and a.logp_backward == b.logp_backward
          and np.array_equal(a.occupancy, b.occupancy) and np.array_equal(a.centre, b.centre))
    if dense:
        ok = ok and a.gamma.shape == b.gamma.shape and np.array_equal(a.gamma, b.gamma)
    return ok


__all__ = ["SCORE_TOL", "GAMMA_TOL", "SUM_RTOL", "fwdbwd_np", "enumerate_np", "window_mask", "yardstick", "check_posteriors",
           "same_bits"]
