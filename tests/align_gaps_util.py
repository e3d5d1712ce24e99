"""Alignment with gaps (BeamSearchDecoderCTC.align_gaps / align_gaps_batch; DESIGN.md "Alignment with gaps"), shared by the CPU
and GPU tests: a float64 Viterbi in numpy over the clipped log-softmax of tests/token_logp_util.lp_matrix with gap slots and
their tie rule -- written from the definition, not from csrc/ctc_align.h --, the gap patterns every shape case runs under, and
the checks every result goes through. As for align, the frames of the yardstick's own path are compared only on planted
inputs, where the margin is nats: on random inputs two optimal paths may tie."""
import numpy as np

from tests.align_util import SCORE_TOL, MAX_LABELS, case_input, random_target, shape_cases, spans_of, viterbi_np
from tests.token_logp_util import FOLDS, fold_of, lp_matrix, tol_of

GAP = -1
PATTERNS = ("none", "leading", "trailing", "both", "every", "middle", "doubled")


def viterbi_gaps_np(lp, target, gaps, blank):
    """The best path for `target` (L >= 1 labels) with gaps[j] saying whether slot j of the L + 1 is a gap, through the [T, V]
    float64 log-probabilities `lp`: (score, path), path holding -1 on the frames of a gap slot. States: slot 0, target[0],
    slot 1, ..., slot L. A label emits lp[t, label], a plain slot lp[t, blank], a gap slot max(lp[t]). A state is entered from
    itself, the state before, or -- a label that differs from the label before it -- two states before; equal scores prefer
    stay, then step, then skip, except in a gap slot, where step is preferred over stay. The last label is preferred over
    the trailing slot. (None, None) when no path exists."""
    T, L = lp.shape[0], len(target)
    assert L >= 1 and len(gaps) == L + 1
    S = 2 * L + 1
    ext = np.full(S, blank, dtype=np.int64)
    ext[1::2] = target
    is_gap = np.zeros(S, dtype=bool)
    is_gap[0::2] = np.asarray(gaps, dtype=bool)
    if T == 0:
        return None, None
    g = lp.max(axis=1)
    can_skip = np.zeros(S, dtype=bool)
    can_skip[3::2] = ext[3::2] != ext[1:-2:2]

    def emit(t):
        e = lp[t, ext].copy()
        e[is_gap] = g[t]
        return e

    score = np.full(S, -np.inf)
    score[:2] = emit(0)[:2]
    back = np.zeros((T, S), dtype=np.int8)
    for t in range(1, T):
        padded = np.concatenate(([-np.inf, -np.inf], score))
        stay, step, skip = score, padded[1:S + 1], np.where(can_skip, padded[:S], -np.inf)
        best, b = stay.copy(), np.zeros(S, dtype=np.int8)
        take = np.where(is_gap, (step >= best) & np.isfinite(step), step > best)
        best, b = np.where(take, step, best), np.where(take, 1, b)
        take = skip > best
        best, b = np.where(take, skip, best), np.where(take, 2, b)
        back[t] = b
        score = best + emit(t)
    s = S - 2 if score[S - 2] >= score[S - 1] else S - 1
    if not np.isfinite(score[s]):
        return None, None
    total = float(score[s])
    path = np.zeros(T, dtype=np.int32)
    for t in range(T - 1, -1, -1):
        path[t] = GAP if is_gap[s] else ext[s]
        s -= int(back[t, s])
    return total, path


def doubled_slot(target):
    """The slot between the first pair of equal neighbours, or None."""
    for k in range(1, len(target)):
        if target[k] == target[k - 1]:
            return k
    return None


def gaps_of_pattern(pattern, target):
    """The L + 1 slot flags of a named pattern, or None where the target has no such slot."""
    L = len(target)
    gaps = [0] * (L + 1)
    if pattern == "leading":
        gaps[0] = 1
    elif pattern == "trailing":
        gaps[L] = 1
    elif pattern == "both":
        gaps[0] = gaps[L] = 1
    elif pattern == "every":
        gaps = [1] * (L + 1)
    elif pattern == "middle":
        if L < 2:
            return None
        gaps[L // 2] = 1
    elif pattern == "doubled":
        k = doubled_slot(target)
        if k is None:
            return None
        gaps[k] = 1
    else:
        assert pattern == "none"
    return gaps


def items_of(target, gaps):
    """The tokens= form: the labels with -1 wherever a slot is a gap."""
    out = []
    for j, c in enumerate(target):
        if gaps[j]:
            out.append(GAP)
        out.append(int(c))
    if gaps[len(target)]:
        out.append(GAP)
    return out


def gap_cases():
    """shape_cases() with at least one label, plus the two sizes at which the kernel's thread count switches."""
    rng = np.random.default_rng(20250)
    cases = [c for c in shape_cases() if len(c[3]) >= 1]
    for L in (511, 512):
        cases.append(("L%d_T1100" % L, 29, 1100, random_target(rng, L, 29, doubled=4), np.float64, "logits"))
    return cases


def g_of(lp):
    return lp.max(axis=1)


def sum_in_order(values):
    acc = 0.0
    for v in values:
        acc += float(v)
    return acc


def check_gapped(a, x, target, gaps, dec, fold=None, what="", plain_score=None, every_score=None, gap_marker="*"):
    """Every property of one GappedAlignment against numpy. `plain_score` / `every_score`: the scores the same library returns
    for the same labels and input without gaps (align) and with every slot a gap (the bounds, compared without a tolerance).
    Returns the yardstick's optimum."""
    labels = dec._alphabet.labels
    blank, space = labels.index(""), (labels.index(" ") if " " in labels and not dec._alphabet.is_bpe else -1)
    xn = np.asarray(x)
    lp = lp_matrix(xn)
    T, L = lp.shape[0], len(target)
    g = g_of(lp)
    path = a.path
    assert path.dtype == np.int32 and path.shape == (T,), (what, path.dtype, path.shape)
    assert a.tokens == items_of(target, gaps), (what, a.tokens)
    # the non-gap runs are the target's labels in order (a gap or a blank separates a doubled label)
    runs = [r for r in spans_of(path, blank) if r[0] != GAP]
    assert [c for c, _, _ in runs] == list(target), (what, [c for c, _, _ in runs], list(target))
    prev_end = 0
    for _c, s, e in runs:
        assert prev_end <= s < e <= T, (what, s, e)
        prev_end = e
    # gaps: the frames between neighbouring labels, all of them -1; -1 nowhere else
    want_gaps = []
    for j in range(L + 1):
        if gaps[j]:
            want_gaps.append((runs[j - 1][2] if j > 0 else 0, runs[j][1] if j < L else T))
    assert a.gaps == want_gaps, (what, a.gaps, want_gaps)
    in_gap = np.zeros(T, dtype=bool)
    for s, e in want_gaps:
        assert 0 <= s <= e <= T, (what, s, e)
        in_gap[s:e] = True
    assert np.array_equal(path == GAP, in_gap), (what, path.tolist(), want_gaps)
    # tokens, words and text as check_aligned derives them; a gap ends a word
    want_tok = [(labels[c], (s, e)) for c, s, e in runs if c != space]
    assert a.token_frames == want_tok, (what, a.token_frames, want_tok)
    words, cur, parts = [], [], []

    def close():
        nonlocal cur
        if cur:
            words.append(cur)
        cur = []

    for j, (c, s, e) in enumerate(runs):
        if gaps[j]:
            close()
            parts.append((gap_marker, len(words)))
        lab = labels[c]
        if c == space or (dec._alphabet.is_bpe and lab.startswith("▁")):
            close()
            if c == space:
                continue
        cur.append((lab.strip("▁"), s, e))
    close()
    if gaps[L]:
        parts.append((gap_marker, len(words)))
    want_words = [("".join(p for p, _, _ in w), (w[0][1], w[-1][2])) for w in words]
    assert a.text_frames == want_words, (what, a.text_frames, want_words)
    pieces = [w for w, _ in want_words]
    for marker, at in reversed(parts):
        pieces.insert(at, marker)
    assert a.text == " ".join(pieces), (what, a.text, pieces)
    # the score: the sum along the path with g(t) on gap frames, and the optimum
    along = sum_in_order(g[t] if c == GAP else lp[t, int(c)] for t, c in enumerate(path))
    best, _ = viterbi_gaps_np(lp, list(target), gaps, blank)
    print("%s: score %.12f, along the path %.12f, numpy optimum %.12f" % (what, a.score, along, best))
    assert abs(a.score - along) <= SCORE_TOL, (what, a.score, along)
    assert abs(a.score - best) <= SCORE_TOL, (what, a.score, best)
    assert len(a.gap_logp) == len(a.gaps)
    for (s, e), got in zip(a.gaps, a.gap_logp):
        want = sum_in_order(g[s:e])
        assert abs(got - want) <= SCORE_TOL, (what, s, e, got, want)
    # the two exact inequalities, without tolerance. The lower bound: align's own score for the labels without the gaps, from
    # the same library. The upper bound: the sum of g(t) over all frames in frame order, from the call's own input. numpy's
    # log-sum-exp (pairwise sums) and the library's (blocks of 16) may differ in the last bit of a row; where a path takes its
    # row's maximum in every frame -- the planted inputs -- that rounding alone can put the score above numpy's sum. Then, and
    # only then, the comparison is made inside the library's own arithmetic instead: against the score of the same call with
    # every slot a gap, whose every emission is >= this call's in the same frame order (`every_score`), and that score in
    # turn lies within the float64 bound of numpy's sum.
    if plain_score is not None:
        print("%s: plain align %.12f <= %.12f" % (what, plain_score, a.score))
        assert a.score >= plain_score, (what, a.score, plain_score)
    upper = sum_in_order(g)
    print("%s: %.17g <= sum of g %.17g (all slots gaps: %s)" % (what, a.score, upper, every_score))
    if every_score is not None:
        assert a.score <= every_score, (what, a.score, every_score)
    if not a.score <= upper:
        assert every_score is not None and every_score <= upper + SCORE_TOL, (what, a.score, upper, every_score)
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


def same_gapped(a, b):
    return (a.text == b.text and a.tokens == b.tokens and np.array_equal(a.path, b.path) and a.score == b.score
            and a.token_frames == b.token_frames and a.text_frames == b.text_frames and a.gaps == b.gaps
            and a.gap_logp == b.gap_logp and a.token_logp == b.token_logp and a.word_logp == b.word_logp)


def equals_plain(a, p):
    """A gap-free GappedAlignment against the AlignedText of align for the same input: exactly."""
    return (a.score == p.score and np.array_equal(a.path, p.path) and a.token_frames == p.token_frames
            and a.text_frames == p.text_frames and a.token_logp == p.token_logp and a.word_logp == p.word_logp
            and a.text == p.text and a.gaps == [] and a.gap_logp == [])


__all__ = ["FOLDS", "SCORE_TOL", "MAX_LABELS", "GAP", "PATTERNS", "viterbi_gaps_np", "gaps_of_pattern", "items_of", "gap_cases",
           "check_gapped", "same_gapped", "equals_plain", "case_input", "viterbi_np", "doubled_slot"]
