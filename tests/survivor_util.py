"""Shared by the CPU (sim) and GPU tests: the frame-prune stage's survivor lists against CPython's own set."""
import ctypes as C

import numpy as np

from oracle.ctc_oracle import normalise_logits
from oracle.np_sum_pieces import rule_whole


def numbered_labels(V):
    """V - 1 distinct labels (the blank makes V) for any V up to 65535: chr(0x4E00 + i) runs into the surrogates there."""
    return ["n%d" % i for i in range(V - 1)]


def telling_rows(rng, V, dtype, n=8, scale=2.0, candidates=48):
    """n rows of logits of which, above 8192 labels, half are ones that TELL numpy's summation order from a single pairwise
    recursion over the row: a last-bit difference in the normaliser reaches its logarithm only about one time in eight (the
    logarithm of a sum near V has an ulp several times the sum's relative one), so rows drawn blindly would let the wrong
    order pass more often than not. Chosen by numpy and a restatement of the recursion alone, never by the code under test.
    float64 rows are, besides, only ones whose normaliser has the same logarithm whether its terms come from numpy's float64
    exp or from libm's (they differ in the last bit of about one argument in twenty where numpy runs its SIMD routine): the
    simulator computes float64 rows with libm, the GPU with ocml, and neither is what this is about."""
    import math

    x = (rng.standard_normal((candidates, V)) * scale).astype(dtype)
    with np.errstate(all="ignore"):
        terms = np.exp(x - x.max(axis=1, keepdims=True))
        assert terms.dtype == dtype
        lse = np.log(terms.sum(axis=1))
        telling = [int(t) for t in np.flatnonzero(np.log(rule_whole(terms)) != lse)] if V > 8192 else []

    def usable(t):
        if dtype != np.float64:
            return True
        libm = np.array([[math.exp(v) for v in x[t] - x[t].max()]])
        return math.log(libm.sum(axis=1)[0]) == lse[t]

    keep = [t for t in telling if usable(t)][: n // 2]
    assert len(keep) >= (1 if V > 8192 else 0), (V, telling)
    for t in range(candidates):
        if len(keep) == n:
            break
        if t not in keep and usable(t):
            keep.append(t)
    assert len(keep) == n
    return np.ascontiguousarray(x[sorted(keep)])


def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch"


def survivors(dec, x, token_min_logp):
    """-> list of (ids, logps) per frame, straight from ctcdec_frame_survivors. `x`: a numpy matrix (staged by the library at
    an aligned device address) or a C-contiguous torch DEVICE tensor, read in place from its own address (bfloat16 included)."""
    if _is_torch(x):
        import torch

        assert x.is_cuda and x.dim() == 2 and x.is_contiguous(), "device tensors: C-contiguous [T, V] on the GPU"
        T, V = x.shape
        dtype = {torch.float32: 0, torch.float64: 1, torch.float16: 2, torch.bfloat16: 3}[x.dtype]
        torch.cuda.synchronize()  # (the library reads on its own stream)
        ptr, is_device = C.c_void_p(x.data_ptr()), 1
    else:
        x = np.ascontiguousarray(x)
        T, V = x.shape
        dtype = {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(np.float16): 2}[x.dtype]
        ptr, is_device = x.ctypes.data_as(C.c_void_p), 0
    counts = np.zeros(max(T, 1), np.int32)
    ids = np.zeros(max(T * V, 1), np.int32)
    lps = np.zeros(max(T * V, 1), np.float64)
    dec._lib.check(dec._lib.dll.ctcdec_frame_survivors(dec._handle, ptr, T, dtype, is_device, float(token_min_logp), V,
                                                        counts.ctypes.data_as(C.POINTER(C.c_int32)),
                                                        ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                                        lps.ctypes.data_as(C.POINTER(C.c_double))))
    return [(ids[t * V:t * V + counts[t]].tolist(), lps[t * V:t * V + counts[t]].tolist()) for t in range(T)]


def as_float64(x):
    """The exact float64 upcast of a numpy matrix or a torch tensor (bfloat16 is not a numpy dtype), as a numpy array."""
    if _is_torch(x):
        return x.detach().double().cpu().numpy()
    return np.asarray(x).astype(np.float64)


def probability_rows(rng, T=6, V=32):
    """Softmax outputs (float64): every row sums to 1, so the prune stage reads them as log(clip(p)) (decoder.py:760-762)."""
    e = np.exp(rng.standard_normal((T, V)) * 2)
    return e / e.sum(axis=1, keepdims=True)


OVERFLOW_TMIN = -2.0
OVERFLOW_BOUND = int(np.floor(np.exp(-OVERFLOW_TMIN))) + 2  # 9: what normalised rows can keep, the width the prune stage first reserves


def overflow_rows(rng, T=6, V=32):
    """Un-normalised non-negative rows whose mean sum is EXACTLY 1 -- read as probabilities -- but whose even rows hold
    more labels above e^OVERFLOW_TMIN = 0.1353 than normalised rows could: ten at 9/64 (row sum 90/64); odd rows four of
    them and one 1/32 (row sum 38/64). Every value and sum is exact in binary floating point."""
    x = np.zeros((T + T % 2, V))
    for t in range(x.shape[0]):
        at = rng.permutation(V)
        if t % 2 == 0:
            x[t, at[:OVERFLOW_BOUND + 1]] = 9 / 64
        else:
            x[t, at[:4]] = 9 / 64
            x[t, at[4]] = 1 / 32
    assert x.sum(axis=1).mean() == 1.0
    return x


def expected_logp(x):
    """The reference's frame log-probabilities for `x` (numpy matrix or torch tensor), widened to float64. float32 rows: the
    product restates the reference's float32 log-softmax (the default, csrc/np_f32.h) -- the oracle's normalisation on the
    float32 matrix itself is then the exact expectation; otherwise the exact float64 upcast."""
    import os

    is32 = str(x.dtype).replace("torch.", "") == "float32"
    exact32 = is32 and os.environ.get("CTCDEC_PRUNE_EXP", "np")[0] == "n"
    host = as_float64(x).astype(np.float32) if exact32 else as_float64(x)  # (float32 -> float64 -> float32: the same bits)
    with np.errstate(all="ignore"):
        return normalise_logits(host).astype(np.float64)


def check_exact(got, lp, token_min_logp, what=""):
    """Survivor lists against log-probabilities `lp` that the stage is meant to reproduce BIT FOR BIT: with equal bits the
    threshold test is decidable, so there is no borderline allowance -- the members are where(lp >= tmin) | {argmax}, in a real
    CPython set's order, and every log-probability is equal."""
    assert len(got) == len(lp), what
    for t, (ids, lps) in enumerate(got):
        row = lp[t]
        # decoder.py:444-445: the set is built from the ascending index array, then `| {argmax}`
        expect = [int(i) for i in set(np.where(row >= token_min_logp)[0]) | {np.argmax(row)}]
        assert ids == expect, (what, t, ids[:20], expect[:20])
        want = row[ids]
        if not np.array_equal(np.asarray(lps), want):
            bad = np.flatnonzero(np.asarray(lps) != want)
            i = int(bad[0])
            raise AssertionError("%s: frame %d: %d of %d log-probabilities differ from the reference's bits, first label %d: %r != %r"
                                 % (what, t, len(bad), len(ids), ids[i], lps[i], float(want[i])))


def check_against_cpython(dec, x, token_min_logp, tol, lp=None):
    """-> the number of border rows. `x`: numpy matrix or torch device tensor; `lp`: the expected log-probabilities when the
    caller already has them (expected_logp(x) otherwise)."""
    got = survivors(dec, x, token_min_logp)
    if lp is None:
        lp = expected_logp(x)
    n_border = 0
    for t, (ids, lps) in enumerate(got):
        row = lp[t]
        # labels whose log-prob sits within tol of the threshold may fall on either side (last-bit exp/log)
        sure = set(int(i) for i in np.where(row >= token_min_logp + tol)[0])
        maybe = set(int(i) for i in np.where(row >= token_min_logp - tol)[0])
        amax = int(np.argmax(row))
        assert sure <= set(ids) <= (maybe | {amax}), (t, ids)
        if abs(row[amax] - token_min_logp) <= tol:  # is argmax in the where-list? undecidable at this tolerance
            n_border += 1
            continue
        # the where-list as the device saw it (borderline labels taken as they fell), argmax only if it passes
        members = set(ids) if row[amax] >= token_min_logp else set(ids) - {amax}
        if members != set(int(i) for i in np.where(row >= token_min_logp)[0]):
            n_border += 1
        # decoder.py:444-445: the set is built from the ascending index array, then `| {argmax}`
        expect = list(set(np.array(sorted(members), dtype=np.int64)) | {np.int64(amax)})
        assert ids == [int(i) for i in expect], (t, ids, expect)
        for i, v in zip(ids, lps):
            assert abs(v - row[i]) <= tol * max(1.0, abs(row[i])), (t, i, v, row[i])
    return n_border
