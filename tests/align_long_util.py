"""Forced alignment of long transcripts (BeamSearchDecoderCTC.align_long / align_long_batch; DESIGN.md "Forced alignment of long
transcripts"), shared by the CPU and GPU tests: the segment lengths every shape case of tests/align_util.py is cut at, the
comparison with align -- equal element for element, bit for bit --, the plan a call must report, the cases above align's 2047
labels that go against the numpy Viterbi, and the mixed batch."""
import numpy as np

from tests.align_util import FOLDS, case_input, char_labels, check_aligned, random_logits, random_target, shape_cases

LONG_MAX_LABELS = 1048575
SHAPES = shape_cases()


def build(V):
    from pyctcdecode_amd import build_ctcdecoder

    return build_ctcdecoder(char_labels(V))


def segment_lengths(name, T):
    """The forced segment lengths of a shape case: the library's own choice, one frame, two, a length that divides nothing,
    one frame short of all, all, more than all. limit_L2047 takes three, to stay within seconds."""
    if name == "limit_L2047":
        return [0, 7, 1000]
    return sorted({0, 1, 2, 7, T + 5} | {k for k in (T - 1, T) if k >= 1})


def plan_of(T, K):
    """What last_align_long_plan holds for an utterance of T frames cut at a forced K (0: whole, the table fits)"""
    if T <= 0:
        return (0, 0)
    k = T if K == 0 else min(K, T)
    return (k, -(-(T - 1) // k))


def same(a, b):
    """Equal element for element, bit for bit (== on floats: no tolerance)"""
    return (a.text == b.text and a.path.dtype == b.path.dtype and np.array_equal(a.path, b.path) and a.score == b.score
            and a.token_frames == b.token_frames and a.text_frames == b.text_frames and a.token_logp == b.token_logp
            and a.word_logp == b.word_logp)


def crosses(a, K):
    """The tokens of an AlignedText whose span holds frames on both sides of a multiple of K"""
    return [(lab, (s, e)) for lab, (s, e) in a.token_frames if (e - 1) // K > s // K]


def check_equals_align(dec, x, target, name, T, inputs=None):
    """align_long == align at every segment length and fold, with the plan that was forced. `inputs`: the forms of x to align
    (host array, device tensor); every form must give the same bits. Returns the results at K = 7 without a fold."""
    inputs = inputs if inputs is not None else [x]
    at7 = None
    for fold in (None,) + FOLDS:
        want = dec.align(x, tokens=target, confidence=fold)
        for K in segment_lengths(name, T):
            for xin in inputs:
                got = dec.align_long_batch([xin], tokens=[target], confidence=fold, _segment_frames=K)[0]
                assert same(got, want), (name, fold, K)
                assert dec.last_align_long_plan == [plan_of(T, K)], (name, K, dec.last_align_long_plan)
                assert dec.last_align_long_launches == (1 if T > 0 else 0), (name, K)
                if K == 7 and fold is None:
                    at7 = got
    return at7


# (name, V, L, T, doubled, dtype): above align's limit, against numpy. nch = ceil((2 L + 1) / 4) is 1025 at L = 2048: the first
# shape at which one of the kernel's 1024 threads owns two groups; 4100 labels give some threads three.
ABOVE = [("L2048_T2100", 5, 2048, 2100, 20, np.float64),
         ("L2049_T2300", 5, 2049, 2300, 0, np.float64),
         ("L4100_T4400", 5, 4100, 4400, 0, np.float64),
         ("V29_L3000_T9000_f32", 29, 3000, 9000, 0, np.float32)]
ABOVE_SEGMENT = 97


def above_input(case):
    name, V, L, T, doubled, dtype = case
    rng = np.random.default_rng(sum(map(ord, name)))
    return random_target(rng, L, V, doubled=doubled), random_logits(rng, T, V, dtype)


def check_above(dec, case, inputs=None):
    """One case above 2047 labels: whole and in segments of 97 frames, equal to each other with ==, and against numpy
    (check_aligned: the path, the sum along it, viterbi_np's optimum within SCORE_TOL, spans, words). Returns the gap to the
    optimum."""
    name, V, L, T, _doubled, _dtype = case
    target, x = above_input(case)
    inputs = inputs if inputs is not None else [x]
    got = []
    for xin in inputs:
        for K in (0, ABOVE_SEGMENT):
            got.append(dec.align_long_batch([xin], tokens=[target], _segment_frames=K)[0])
            assert dec.last_align_long_plan == [plan_of(T, K)], (name, K, dec.last_align_long_plan)
    assert all(same(got[0], g) for g in got[1:]), name
    best = check_aligned(got[0], x, target, dec, None, name)
    gap = abs(got[0].score - best)
    print("%s: |score - numpy optimum| = %.3e" % (name, gap))
    return gap


def mixed_batch():
    """(xs, targets, infeasible index): float64 utterances over 29 labels -- shapes of the cases above and below 2047 labels,
    no frames, no labels, and one utterance with fewer frames than its target needs."""
    rng = np.random.default_rng(77)
    V = 29
    shapes = [(300, 127, 4), (0, 0, 0), (9, 0, 0), (2300, 2049, 0), (40, 11, 1), (1, 1, 0), (5, 9, 0), (300, 32, 4), (64, 30, 2)]
    xs, targets = [], []
    for T, L, doubled in shapes:
        xs.append(random_logits(rng, T, V))
        targets.append(random_target(rng, L, V, doubled=doubled) if L else [])
    return xs, targets, 6


__all__ = ["ABOVE", "ABOVE_SEGMENT", "FOLDS", "LONG_MAX_LABELS", "SHAPES", "above_input", "build", "case_input", "check_above",
           "check_equals_align", "crosses", "mixed_batch", "plan_of", "same", "segment_lengths"]
