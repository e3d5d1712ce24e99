"""Greedy best-path decoding (BeamSearchDecoderCTC.decode_greedy / decode_greedy_batch; DESIGN.md "Greedy decode"), shared by the
CPU and GPU tests: the definition restated in numpy -- a NaN-aware argmax that takes the smallest index, the blank rule, the
collapse of runs, the confidences from tests/token_logp_util.lp_matrix --, the checks every result goes through, and the
inputs of the cases: planted ties, NaN / -inf rows and label sequences laid around the 64-frame step of greedy_collapse."""
import math

import numpy as np

from tests.align_util import SCORE_TOL, char_labels, random_logits
from tests.token_logp_util import LOGP_FLOOR, fold_of, lp_matrix, tol_of

VOCABS = (29, 131, 300, 1024)  # 4, 16, 16 and 64 lanes per row; 131: rows off a 16-byte boundary, elements left over
FRAMES = (0, 1, 63, 64, 65, 129)
BLANK, SPACE = 0, 1  # of char_labels(V)


def build(V):
    from pyctcdecode_amd import build_ctcdecoder

    return build_ctcdecoder(char_labels(V))


def argmax_np(x, blank):
    """Per row the smallest index among the entries equal to the row's largest entry that is not a NaN; the blank for a row
    without an entry above -inf. (-0.0 == +0.0 in numpy as on the device.)"""
    xd = np.asarray(x).astype(np.float64)
    out = np.full(len(xd), blank, dtype=np.int32)
    for t, row in enumerate(xd):
        row = np.where(np.isnan(row), -np.inf, row)
        m = row.max() if len(row) else -np.inf
        if m > -np.inf:
            out[t] = int(np.flatnonzero(row == m)[0])
    return out


def collapse_np(arg, blank):
    """(label, start, end) of every maximal run of one label other than the blank, end exclusive."""
    out, t, T = [], 0, len(arg)
    while t < T:
        c, e = int(arg[t]), t + 1
        while e < T and int(arg[e]) == c:
            e += 1
        if c != blank:
            out.append((c, t, e))
        t = e
    return out


def emissions_np(x, arg):
    """e(t): the clipped float64 log-probability of row t's label -- a column of lp_matrix; where the matrix holds NaN or -inf
    (logits, then) the log-softmax of each row with a maximum, a NaN counting as -inf as in the device's log-sum-exp, and the
    floor for a row without one."""
    xn = np.asarray(x)
    e = np.full(len(xn), LOGP_FLOOR)
    if xn.size == 0:
        return e
    if np.isfinite(xn).all():
        return lp_matrix(xn)[np.arange(len(xn)), arg]
    clean = np.where(np.isnan(xn), -np.inf, xn).astype(np.float64)
    rows = np.flatnonzero(clean.max(axis=1) > -np.inf)
    xd = clean[rows]
    m = xd.max(axis=1, keepdims=True)
    lse = m + np.log(np.exp(xd - m).sum(axis=1, keepdims=True))
    e[rows] = np.clip(xd - lse, LOGP_FLOOR, 0)[np.arange(len(rows)), arg[rows]]
    return e


def check_greedy(g, x, dec, fold=None, what=""):
    """Every field of one GreedyText against numpy."""
    labels = dec._alphabet.labels
    blank = labels.index("")
    space = labels.index(" ") if " " in labels and not dec._alphabet.is_bpe else -1
    arg = argmax_np(x, blank)
    runs = collapse_np(arg, blank)
    assert g.tokens == [c for c, _, _ in runs], (what, g.tokens, runs)
    assert g.token_frames == [(labels[c], (s, e)) for c, s, e in runs if c != space], (what, g.token_frames)
    text, kept, words = dec._words_of_target(g.tokens)
    assert g.text == text, (what, g.text, text)
    spans = [(s, e) for c, s, e in runs if c != space]
    assert g.text_frames == [(w, (spans[lo][0], spans[hi - 1][1])) for w, lo, hi in words], (what, g.text_frames)
    if fold is None:
        assert g.token_logp is None and g.word_logp is None and g.score is None, what
        return arg
    e = emissions_np(x, arg)
    tol = tol_of(np.asarray(x).dtype)
    assert len(g.token_logp) == len(g.token_frames) and len(g.word_logp) == len(g.text_frames), what
    for (lab, (s, t1)), got in zip(g.token_frames, g.token_logp):
        want = fold_of(e[s:t1], fold)
        print("%s: token %r [%d, %d) logp %.12f numpy %.12f" % (what, lab, s, t1, got, want))
        assert abs(got - want) <= tol, (what, lab, s, t1, got, want)
    for (_w, lo, hi), got in zip(words, g.word_logp):
        assert got == min(g.token_logp[lo:hi]), (what, got)
    along = 0.0
    for v in e.tolist():
        along += v
    print("%s: score %.12f numpy %.12f" % (what, g.score, along))
    assert math.isfinite(g.score) and abs(g.score - along) <= SCORE_TOL, (what, g.score, along)
    return arg


def same_greedy(a, b):
    return (a.text == b.text and a.tokens == b.tokens and a.token_frames == b.token_frames and a.text_frames == b.text_frames and
            a.token_logp == b.token_logp and a.word_logp == b.word_logp and a.score == b.score)


def of_batch(texts, frames, u, dec):
    """Utterance u of a decode_greedy_batch result, in the shape same_batch_entry compares with a GreedyText."""
    return texts[u], frames.of(u), (frames.logp_of(u) if frames.logp is not None else None), (
        float(frames.score[u]) if frames.score is not None else None)


def same_batch_entry(entry, g):
    text, tok, logp, score = entry
    return text == g.text and tok == g.token_frames and logp == g.token_logp and score == g.score


def logits_of_labels(seq, V, rng, dtype=np.float64):
    """A [T, V] matrix of small integers (exact in every dtype) whose row t has its only maximum at seq[t]."""
    x = rng.integers(-8, 0, size=(len(seq), V)).astype(np.float64)
    if len(seq):
        x[np.arange(len(seq)), np.asarray(seq, dtype=np.int64)] = 4.0
    return x.astype(dtype)


def collapse_sequences(a=5, b=7):
    """name -> label sequence: what can go wrong in greedy_collapse's 64-frame steps."""
    seqs = {}
    for T in FRAMES:
        seqs["T%d_one_label" % T] = [a] * T                             # a token that runs to the last frame
        seqs["T%d_all_blank" % T] = [BLANK] * T
        seqs["T%d_alternating" % T] = [a if t % 2 == 0 else b for t in range(T)]  # T tokens: the maximum
        seqs["T%d_blank_between" % T] = [a if t % 2 == 0 else BLANK for t in range(T)]
    s = [BLANK] * 129
    s[60:70] = [a] * 10
    seqs["run_crosses_63_64"] = list(s)
    s = [BLANK] * 129
    s[62:64], s[64:66] = [a, a], [b, b]
    seqs["ends_on_63_starts_on_64"] = list(s)
    s = [BLANK] * 129
    s[62], s[64] = a, a
    seqs["a_blank_then_a_across"] = list(s)
    s = [BLANK] * 129
    s[62:66] = [a] * 4
    seqs["aa_aa_across"] = list(s)
    s = [BLANK] * 129
    s[63], s[64], s[127], s[128] = a, b, a, a
    seqs["last_lane_first_lane_and_the_end"] = list(s)
    s = [a] * 129
    s[64] = BLANK
    seqs["blank_on_64_alone"] = list(s)
    return seqs


def tie_pairs(V, itemsize):
    """(i, j), i < j: where a row holds its maximum twice -- inside one 16-byte vector, in two lanes' vectors, in a vector and
    in the elements left over after the last whole vector, far apart, and first / last."""
    epv = 16 // itemsize
    pairs = [(0, 1), (epv, 2 * epv + 1), (2, V // 2), (0, V - 1), (V - 2, V - 1), (epv - 1, epv)]
    nvec = V // epv
    if V % epv:
        pairs += [(5, V - 1), (nvec * epv - 1, nvec * epv)]
    if nvec > 64 * 4:  # (a lane's second pass over the row)
        pairs.append((3, (64 * 4 + 1) * epv))
    return [(i, j) for i, j in pairs if 0 <= i < j < V]


def tie_rows(V, dtype_itemsize, rng):
    """-> (x float64 [2 P + 4, V] of small integers and zeros, want [rows]): every pair planted in an even row, the rows between
    them blank; then +0.0 before -0.0 and -0.0 before +0.0 as the maxima of rows of negative entries."""
    pairs = tie_pairs(V, dtype_itemsize)
    T = 2 * len(pairs) + 4
    x = rng.integers(-8, 0, size=(T, V)).astype(np.float64)
    x[1::2, BLANK] = 4.0
    want = np.full(T, BLANK, dtype=np.int32)
    for k, (i, j) in enumerate(pairs):
        x[2 * k, i] = x[2 * k, j] = 4.0
        want[2 * k] = i
    z = 2 * len(pairs)
    i, j = 3, V - 2
    x[z, i], x[z, j] = 0.0, -0.0
    x[z + 2, i], x[z + 2, j] = -0.0, 0.0
    want[z] = want[z + 2] = i
    return x, want


def special_rows(V, rng):
    """-> (x float64 [T, V], want labels): a NaN at index 0 with the maximum elsewhere, NaNs around the maximum, a row of NaN, a
    row of -inf, a row that mixes the two, each between ordinary rows."""
    x = random_logits(rng, 11, V)
    want = argmax_np(x, BLANK)
    x[1, 0], x[1, 9] = np.nan, 50.0
    x[3, :] = np.nan
    x[5, :] = -np.inf
    x[7, ::2], x[7, 1::2] = np.nan, -np.inf
    x[9, 4], x[9, 6], x[9, 5] = np.nan, np.nan, 50.0
    want[[1, 3, 5, 7, 9]] = [9, BLANK, BLANK, BLANK, 5]
    return x, want


def probability_rows(T, V, rng):
    """Powers of two that sum to exactly 1 in every dtype and every order of summation (tests/test_gpu_align_gaps.py)."""
    p = np.zeros((T, V))
    for t in range(T):
        cols = rng.choice(V, size=10, replace=False)
        p[t, cols] = [2.0 ** -k for k in range(1, 10)] + [2.0 ** -9]
    return p


def unique_maxima(x):
    """The premise of the path identities: numpy says every row's two largest entries differ."""
    top = np.sort(np.asarray(x).astype(np.float64), axis=1)[:, -2:]
    return bool((top[:, 1] > top[:, 0]).all())
