"""How numpy adds up a long contiguous row: the experiment behind csrc/np_sum.h.

Candidate rules are restated here in plain numpy scalar arithmetic (vectorised ACROSS rows only: every row sees the very
additions, in the very order, of the rule) and compared bit for bit with the three call forms the reference decoder uses --
`x.sum(axis=1)` (the probabilities-or-logits sniff), `np.sum(x, axis=1, keepdims=True)` (the log-softmax normaliser) and the
row-by-row `x[t].sum()` -- for float32, float64 and float16 rows on both sides of every multiple of numpy's buffer size up to
65535 elements, many random rows per length (a last-bit difference shows in only a fraction of the rows).

  whole : one pairwise recursion over the whole row (numpy's pairwise_sum: leaves of <= 128 elements with eight strided
          accumulators, halves split at n/2 rounded down to a multiple of 8)
  pieces: the row cut into pieces of np.getbufsize() = 8192 elements; each piece summed by that recursion; the pieces' sums added
          to the result one after the other, left to right (float16: the recursion accumulates in float32, and the running
          result is rounded to float16 after EVERY piece -- it lives in the float16 output element between the inner-loop calls)

    python -m oracle.np_sum_pieces            # prints one line per dtype and length: rows that differ from each rule
"""
import sys

import numpy as np


def pairwise(a, acc):
    """numpy's pairwise sum over axis 1 of a [R, n] matrix, in accumulator dtype `acc`; -> [R]"""
    n = a.shape[1]
    if n < 8:
        res = np.zeros(a.shape[0], acc)
        for i in range(n):
            res = res + a[:, i].astype(acc)
        return res
    if n <= 128:
        r = [a[:, j].astype(acc) for j in range(8)]
        body = n - n % 8
        for i in range(8, body, 8):
            for j in range(8):
                r[j] = r[j] + a[:, i + j].astype(acc)
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for i in range(body, n):
            res = res + a[:, i].astype(acc)
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return pairwise(a[:, :n2], acc) + pairwise(a[:, n2:], acc)


def rule_whole(x):
    acc = np.float32 if x.dtype == np.float16 else x.dtype.type
    return pairwise(x, acc).astype(x.dtype)


def rule_pieces(x, piece=None):
    piece = piece or np.getbufsize()
    acc = np.float32 if x.dtype == np.float16 else x.dtype.type
    out = None
    for p in range(0, x.shape[1], piece):
        s = pairwise(x[:, p:p + piece], acc)
        # the running result sits in the output element (of the row's dtype) between pieces
        out = s.astype(x.dtype) if out is None else (out.astype(acc) + s).astype(x.dtype)
    return out


def lengths(limit=65535, piece=8192):
    out = [5000, 7688, 7689, 8200, 20000]
    for k in range(piece, limit + 1, piece):
        out += [k - 1, k, k + 1]
    out.append(limit)
    return sorted(set(n for n in out if n <= limit))


def study(rows=96, seed=11, out=sys.stdout):
    rng = np.random.default_rng(seed)
    bad = 0
    print("numpy %s, bufsize %d; %d rows per length; rows whose sum differs from each rule" % (np.__version__, np.getbufsize(), rows), file=out)
    print("dtype    length  forms_agree  whole  pieces", file=out)
    for dtype in (np.float32, np.float64, np.float16):
        for n in lengths():
            # exponentials of shifted logits (the normaliser's terms) in the upper rows, signed values in the lower ones
            x = rng.standard_normal((rows, n)) * 2
            x[: rows // 2] = np.exp(x[: rows // 2] - x[: rows // 2].max(axis=1, keepdims=True))
            if dtype == np.float16:
                x *= 0.05  # (keep the float16 sums finite)
            x = np.ascontiguousarray(x.astype(dtype))
            a = x.sum(axis=1)
            b = np.sum(x, axis=1, keepdims=True)[:, 0]
            c = np.array([x[t].sum() for t in range(rows)], dtype=dtype)
            agree = np.array_equal(a, b) and np.array_equal(a, c)
            dw = int((rule_whole(x) != a).sum())
            dp = int((rule_pieces(x) != a).sum())
            bad += dp + (not agree)
            print("%-8s %6d  %-11s  %5d  %6d" % (np.dtype(dtype).name, n, agree, dw, dp), file=out)
    # the mean of the row sums (decoder.py:760) reduces a column of T sums the same way: more than 8192 frames
    for dtype in (np.float32, np.float64):
        for T in (8191, 8193, 20000):
            s = rng.standard_normal((4, T)).astype(dtype)
            want = np.array([row.mean() for row in s])
            got = rule_pieces(s) / dtype(T)
            bad += int((got != want).sum())
            print("mean of %d %s sums: %d of 4 differ from pieces / T" % (T, np.dtype(dtype).name, int((got != want).sum())), file=out)
    print("rows that differ from the piece rule, or forms that disagree: %d" % bad, file=out)
    return bad


if __name__ == "__main__":
    sys.exit(1 if study() else 0)
