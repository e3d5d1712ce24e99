"""Forced alignment (BeamSearchDecoderCTC.align / align_batch; DESIGN.md "Forced alignment"), shared by the CPU and GPU tests:
a textbook float64 Viterbi in numpy over the clipped log-softmax of tests/token_logp_util.lp_matrix -- written from the
definition, not from csrc/ctc_align.h --, the checks every case goes through, and the list of cases. The frames of the
yardstick's own path are never compared: two optimal paths may tie, and the checks hold whichever one is returned."""
import numpy as np

from tests.token_logp_util import FOLDS, fold_of, lp_matrix, tol_of

SCORE_TOL = 1e-9  # float64 scores: the bound smoke() and the fp64 parity tests use
MAX_LABELS = 2047


def viterbi_np(lp, target, blank):
    """The best CTC path for `target` through the [T, V] float64 log-probabilities `lp`: (score, path). States are
    blank, target[0], blank, target[1], ..., blank; a state is entered from itself, from the state before, or -- a label
    that differs from the label before it -- from two states before. Returns (None, None) when no path exists."""
    T, L = lp.shape[0], len(target)
    ext = np.full(2 * L + 1, blank, dtype=np.int64)
    ext[1::2] = target
    S = len(ext)
    if T == 0:
        return (0.0, np.zeros(0, dtype=np.int32)) if L == 0 else (None, None)
    can_skip = np.zeros(S, dtype=bool)
    can_skip[3::2] = ext[3::2] != ext[1:-2:2]
    score = np.full(S, -np.inf)
    score[0] = lp[0, blank]
    if L:
        score[1] = lp[0, ext[1]]
    back = np.zeros((T, S), dtype=np.int8)
    for t in range(1, T):
        stay = score
        padded = np.concatenate(([-np.inf, -np.inf], score))
        step = padded[1:S + 1]
        skip = np.where(can_skip, padded[:S], -np.inf)
        cand = np.stack([stay, step, skip])
        back[t] = np.argmax(cand, axis=0)
        score = cand.max(axis=0) + lp[t, ext]
    s = S - 1 if L == 0 or score[S - 1] > score[S - 2] else S - 2
    if not np.isfinite(score[s]):
        return None, None
    best = float(score[s])
    path = np.zeros(T, dtype=np.int32)
    for t in range(T - 1, -1, -1):
        path[t] = ext[s]
        s -= int(back[t, s])
    return best, path


def feasible(T, target):
    return T >= len(target) + sum(1 for a, b in zip(target, target[1:]) if a == b)


def collapse(path, blank):
    out, prev = [], None
    for c in path.tolist():
        if c != prev and c != blank:
            out.append(c)
        prev = c
    return out


def spans_of(path, blank):
    """(label, start, end) of every run of a non-blank label in `path` (a run ends at a blank or at another label)."""
    out, t, T = [], 0, len(path)
    while t < T:
        c = int(path[t])
        e = t + 1
        while e < T and path[e] == c:
            e += 1
        if c != blank:
            out.append((c, t, e))
        t = e
    return out


def check_aligned(a, x, target, dec, fold=None, what=""):
    """Every property of one AlignedText against numpy: the path is a valid alignment of `target`, its score is the sum
    along it and the optimum, spans / words / confidences follow from the path. Returns the yardstick's score."""
    labels = dec._alphabet.labels
    blank, space = labels.index(""), (labels.index(" ") if " " in labels and not dec._alphabet.is_bpe else -1)
    xn = np.asarray(x)
    lp = lp_matrix(xn)
    T = lp.shape[0]
    path = a.path
    assert path.dtype == np.int32 and path.shape == (T,), (what, path.dtype, path.shape)
    assert collapse(path, blank) == list(target), (what, collapse(path, blank), list(target))
    along = float(sum(lp[t, int(c)] for t, c in enumerate(path)))
    print("%s: score %.12f, along the path %.12f" % (what, a.score, along))
    assert abs(a.score - along) <= SCORE_TOL, (what, a.score, along)
    best, _ = viterbi_np(lp, list(target), blank)
    print("%s: numpy optimum %.12f" % (what, best))
    assert abs(a.score - best) <= SCORE_TOL, (what, a.score, best)
    runs = spans_of(path, blank)
    assert [c for c, _, _ in runs] == list(target)  # (one run per target label: a doubled label has a blank between)
    prev_end = 0
    for _c, s, e in runs:
        assert prev_end <= s < e <= T, (what, s, e)
        prev_end = e
    want_tok = [(labels[c], (s, e)) for c, s, e in runs if c != space]
    assert a.token_frames == want_tok, (what, a.token_frames, want_tok)
    # words: the runs between space labels (character alphabets) / from one word-initial piece to the next (BPE)
    words, cur = [], []
    for c, s, e in runs:
        lab = labels[c]
        if c == space or (dec._alphabet.is_bpe and lab.startswith("▁")):
            if cur:
                words.append(cur)
            cur = []
            if c == space:
                continue
        cur.append((lab.strip("▁"), s, e))
    if cur:
        words.append(cur)
    want_words = [("".join(p for p, _, _ in w), (w[0][1], w[-1][2])) for w in words]
    assert a.text_frames == want_words, (what, a.text_frames, want_words)
    assert a.text == " ".join(w for w, _ in want_words), (what, a.text)
    if fold is None:
        assert a.token_logp is None and a.word_logp is None
        return best
    tol = tol_of(xn.dtype)
    index = {lab: c for c, lab in enumerate(labels)}
    assert len(a.token_logp) == len(a.token_frames) and len(a.word_logp) == len(a.text_frames)
    for (lab, (s, e)), got in zip(a.token_frames, a.token_logp):
        want = fold_of(lp[s:e, index[lab]], fold)
        assert abs(got - want) <= tol, (what, lab, s, e, got, want)
    k = 0
    for (_w, (ws, we)), got in zip(a.text_frames, a.word_logp):
        run = []
        while k < len(a.token_frames) and a.token_frames[k][1][1] <= we:
            run.append(a.token_logp[k])
            k += 1
        assert run and got == min(run), (what, ws, we, got, run)
    return best


def char_labels(V):
    """A character alphabet of V labels: the blank, the space, then V - 2 distinct single characters."""
    pool = list("abcdefghijklmnopqrstuvwxyz'") + [chr(0x4E00 + i) for i in range(max(0, V - 29))]
    return ["", " "] + pool[: V - 2]


def random_target(rng, L, V, doubled=0):
    """L label ids in [2, V) (neither blank nor space), `doubled` of them equal to their predecessor."""
    t = rng.integers(2, V, size=L).tolist()
    for k in range(1, L):
        while t[k] == t[k - 1]:
            t[k] = int(rng.integers(2, V))
    for k in rng.choice(np.arange(1, L), size=doubled, replace=False).tolist() if doubled else []:
        t[k] = t[k - 1]
    return t


def random_logits(rng, T, V, dtype=np.float64, scale=3.0):
    return (rng.standard_normal((T, V)) * scale).astype(dtype)


def shape_cases():
    """(name, V, T, target ids, dtype, kind): the smallest shapes at which the recursion or the launch can go wrong.
    kind 'logits' | 'probs' (softmax taken first) | 'ties' (float16 rows with exactly equal maxima)."""
    rng = np.random.default_rng(20241)
    cases = [("T1_L1", 5, 1, [2], np.float64, "logits"),
             ("T_eq_L_no_blanks", 29, 12, random_target(rng, 12, 29), np.float64, "logits"),
             ("empty_target", 5, 7, [], np.float64, "logits"),
             ("T0", 5, 0, [], np.float64, "logits"),
             ("hello_at_bound", 29, 6, [9, 6, 13, 13, 16], np.float32, "logits"),     # h e l l o: 5 labels + 1 repeat
             ("aaa_at_bound", 5, 5, [2, 2, 2], np.float64, "logits"),
             ("limit_L2047", 5, 2100, random_target(rng, MAX_LABELS, 5, doubled=20), np.float64, "logits"),
             ("V1024_f32", 1024, 60, random_target(rng, 17, 1024), np.float32, "logits"),
             ("V130_f16", 130, 50, random_target(rng, 20, 130, doubled=3), np.float16, "logits"),
             ("V29_probs", 29, 40, random_target(rng, 11, 29, doubled=1), np.float64, "probs"),
             ("V29_f16_ties", 29, 30, random_target(rng, 9, 29, doubled=1), np.float16, "ties")]
    for L in (31, 32, 127, 128, 129):  # 2 L + 1 states across the 64-lane and 256-thread boundaries
        cases.append(("L%d_T300" % L, 29, 300, random_target(rng, L, 29, doubled=4), np.float64, "logits"))
    return cases


def case_input(case):
    name, V, T, target, dtype, kind = case
    rng = np.random.default_rng(sum(map(ord, name)))
    x = random_logits(rng, T, V, np.float64)
    if kind == "probs":
        e = np.exp(x - x.max(axis=1, keepdims=True))
        x = e / e.sum(axis=1, keepdims=True)
    elif kind == "ties":
        x = np.round(x)  # small integers, exact in float16: many rows hold their maximum twice
        x[::2, 3] = x[::2].max(axis=1)
        x[::2, 4] = x[::2].max(axis=1)
    return x.astype(dtype)


__all__ = ["FOLDS", "SCORE_TOL", "MAX_LABELS", "viterbi_np", "feasible", "check_aligned", "char_labels", "random_target",
           "random_logits", "shape_cases", "case_input", "collapse", "spans_of"]
