"""CTC prefix scores (BeamSearchDecoderCTC.prefix_scores / prefix_scores_batch; DESIGN.md "Prefix scores"), shared by the CPU
and GPU tests: the definition in numpy float64, in log-sum-exp form over the clipped log-softmax of
tests/token_logp_util.lp_matrix -- written from the definition, not from csrc/ctc_align.h --, the enumeration of all paths it
is checked against, and the checks every result goes through."""
import itertools
import math

import numpy as np

from tests.align_util import SCORE_TOL, feasible
from tests.token_logp_util import lp_matrix

PREFIX_K = 8      # PREFIX_K of csrc/ctc_align.h: prefixes of an utterance that share a read of its rows
PREFIX_SEG = 128  # PREFIX_SEG: frames of a segment
PREFIX_FUSE_BLOCKS = 1024  # PREFIX_FUSE_BLOCKS: (chunk, 256-column tile) pairs from which a launch is not split by segments


def lse(values):
    values = [v for v in values if v > -np.inf]
    if not values:
        return -np.inf
    m = max(values)
    return m + math.log(math.fsum(math.exp(v - m) for v in values))


def alphas_np(lp, prefix, blank):
    """[T, S] the forward recursion of tests/score_util.forward_np, every frame kept (a_t[s] includes frame t's emission)."""
    T, L = lp.shape[0], len(prefix)
    ext = np.full(2 * L + 1, blank, dtype=np.int64)
    ext[1::2] = prefix
    S = len(ext)
    can_skip = np.zeros(S, dtype=bool)
    can_skip[3::2] = ext[3::2] != ext[1:-2:2]
    out = np.full((T, S), -np.inf)
    if T == 0:
        return out
    out[0, 0] = lp[0, blank]
    if L:
        out[0, 1] = lp[0, ext[1]]
    with np.errstate(invalid="ignore"):
        for t in range(1, T):
            alpha = out[t - 1]
            padded = np.concatenate(([-np.inf, -np.inf], alpha))
            acc = np.logaddexp(alpha, padded[1:S + 1])
            acc = np.logaddexp(acc, np.where(can_skip, padded[:S], -np.inf))
            out[t] = acc + lp[t, ext]
    return out


def prefix_of_lp(lp, prefix, blank):
    """(end, next[V]) of the definition, from [T, V] float64 log-probabilities."""
    T, V = lp.shape
    L = len(prefix)
    S = 2 * L + 1
    a = alphas_np(lp, prefix, blank)

    def ends(t):  # lse2(a_t[S-1], a_t[S-2]), and a_t[S-1]
        return (lse([a[t, S - 1], a[t, S - 2]]) if L else a[t, 0]), a[t, S - 1]

    if T == 0:
        return (0.0 if L == 0 else -np.inf), np.full(V, -np.inf)
    end = ends(T - 1)[0]
    A = [0.0 if L == 0 else -np.inf] + [ends(t - 1)[0] for t in range(1, T)]
    B = [-np.inf] + [ends(t - 1)[1] for t in range(1, T)]
    nxt = np.full(V, -np.inf)
    for c in range(V):
        if c == blank:
            continue
        W = B if L and c == prefix[-1] else A
        nxt[c] = lse([W[t] + lp[t, c] for t in range(T)])
    return float(end), nxt


def prefix_np(x, prefix, blank):
    """(end, next[V]) for an input as the library takes it: the emissions are the other utilities' (lp_matrix)."""
    x = np.asarray(x)
    if len(x) == 0:
        return (0.0 if len(prefix) == 0 else -np.inf), np.full(x.shape[1], -np.inf)
    with np.errstate(invalid="ignore"):
        lp = lp_matrix(x)
    lp[np.isnan(lp)] = np.log(1e-15)  # (a row of NaN and -inf alone has no log-sum-exp: its entries take the floor, as a NaN does)
    return prefix_of_lp(lp, list(prefix), blank)


def collapse(seq, blank):
    out, prev = [], None
    for c in seq:
        if c != prev and c != blank:
            out.append(c)
        prev = c
    return out


def prefix_bruteforce(lp, prefix, blank):
    """(end, next[V]) by enumeration of all V^T paths (and of their beginnings): end sums the whole paths that collapse to the
    prefix; next[c] sums, over every frame t, the beginnings of t + 1 frames that collapse to prefix + [c] and whose first t
    frames collapse to the prefix alone -- c first completed at t. A beginning counts up to that frame only, so the sums
    are right for rows that do not sum to 1 too; for rows that do, next[c] is the mass of all whole paths that start so."""
    T, V = lp.shape
    prefix = list(prefix)
    p = np.exp(lp)
    end = 0.0
    nxt = np.zeros(V)
    for n in range(1, T + 1):
        for seq in itertools.product(range(V), repeat=n):
            mass = 1.0
            for t, c in enumerate(seq):
                mass *= p[t, c]
            got = collapse(seq, blank)
            if n == T and got == prefix:
                end += mass
            c = seq[-1]
            if c != blank and got == prefix + [c] and collapse(seq[:-1], blank) == prefix:
                nxt[c] += mass
    if T == 0:
        end = 1.0 if not prefix else 0.0
    with np.errstate(divide="ignore"):
        return float(np.log(end)), np.log(nxt)


def next_array(r):
    """A PrefixScores' next_logp on the host"""
    nxt = r.next_logp
    return nxt.cpu().numpy() if hasattr(nxt, "cpu") else np.asarray(nxt)


def check_prefix(r, x, prefix, blank, what=""):
    """One PrefixScores against prefix_np: within SCORE_TOL wherever both are finite, -inf exactly where the oracle has it."""
    want_end, want_next = prefix_np(x, prefix, blank)
    got_next = next_array(r)
    assert r.tokens == list(prefix), (what, r.tokens)
    assert got_next.dtype == np.float64 and got_next.shape == want_next.shape, (what, got_next.dtype, got_next.shape)
    fin = np.isfinite(want_next)
    worst = float(np.abs(got_next[fin] - want_next[fin]).max()) if fin.any() else 0.0
    print("%s: end %.12f (numpy %.12f), next: %d finite, worst difference %.3e" % (what, r.logp_end, want_end, int(fin.sum()), worst))
    if math.isinf(want_end):
        assert r.logp_end == want_end, (what, r.logp_end, want_end)
    else:
        assert abs(r.logp_end - want_end) <= SCORE_TOL, (what, r.logp_end, want_end)
    assert np.array_equal(np.isneginf(got_next), np.isneginf(want_next)), (what, np.flatnonzero(np.isneginf(got_next) != np.isneginf(want_next)))
    assert not np.isnan(got_next).any() and got_next[blank] == -np.inf, what
    assert worst <= SCORE_TOL, (what, worst)


def same_prefix(a, b):
    """Bit for bit"""
    return a.text == b.text and a.tokens == b.tokens and a.logp_end == b.logp_end and np.array_equal(next_array(a), next_array(b))


def close_prefix(a, b, tol=1e-9):
    """Two builds of the same call: finite values within tol, -inf in the same places"""
    na, nb = next_array(a), next_array(b)
    if a.tokens != b.tokens or a.text != b.text or not np.array_equal(np.isneginf(na), np.isneginf(nb)):
        return False
    fin = np.isfinite(na)
    if (~fin & ~np.isneginf(na)).any() or (fin.any() and np.abs(na[fin] - nb[fin]).max() > tol):
        return False
    if math.isinf(a.logp_end) or math.isinf(b.logp_end):
        return a.logp_end == b.logp_end
    return abs(a.logp_end - b.logp_end) <= tol


__all__ = ["SCORE_TOL", "PREFIX_K", "PREFIX_SEG", "PREFIX_FUSE_BLOCKS", "lse", "alphas_np", "prefix_of_lp", "prefix_np",
           "prefix_bruteforce", "next_array", "check_prefix", "same_prefix", "close_prefix", "feasible"]
