"""Transcript likelihood (BeamSearchDecoderCTC.score / score_batch; DESIGN.md "Transcript likelihood"), shared by the CPU and
GPU tests: a textbook float64 CTC forward recursion in numpy over the clipped log-softmax of tests/token_logp_util.lp_matrix --
written from the definition (Graves et al. 2006, eq. 6-8, in log space with np.logaddexp), not from csrc/ctc_align.h --, and
the inputs of the cases tests/align_util.shape_cases() does not have."""
import itertools

import numpy as np

from tests.align_util import SCORE_TOL, case_input, feasible, random_logits, random_target, shape_cases
from tests.token_logp_util import lp_matrix

# the shape cases whose target has exactly one alignment: the forward score is the best path's
SINGLE_PATH = ("T1_L1", "T_eq_L_no_blanks", "empty_target", "hello_at_bound", "aaa_at_bound")
WAVE_MAX_LABELS = 127  # FORWARD_WAVE_MAX_LABELS of csrc/ctc_align.h


def forward_np(lp, target, blank):
    """log of the sum, over every alignment of `target` to the T frames, of the product of the frames' probabilities
    exp(lp[t, label]); -inf when there is no alignment, 0.0 for the empty target without frames."""
    T, L = lp.shape[0], len(target)
    if T == 0:
        return 0.0 if L == 0 else -np.inf
    ext = np.full(2 * L + 1, blank, dtype=np.int64)
    ext[1::2] = target
    S = len(ext)
    can_skip = np.zeros(S, dtype=bool)
    can_skip[3::2] = ext[3::2] != ext[1:-2:2]
    alpha = np.full(S, -np.inf)
    alpha[0] = lp[0, blank]
    if L:
        alpha[1] = lp[0, ext[1]]
    with np.errstate(invalid="ignore"):  # (logaddexp(-inf, -inf) is -inf; numpy computes -inf - -inf on the way)
        for t in range(1, T):
            padded = np.concatenate(([-np.inf, -np.inf], alpha))
            acc = np.logaddexp(alpha, padded[1:S + 1])
            acc = np.logaddexp(acc, np.where(can_skip, padded[:S], -np.inf))
            alpha = acc + lp[t, ext]
        return float(np.logaddexp(alpha[S - 1], alpha[S - 2]) if L else alpha[S - 1])


def yardstick(x, target, blank):
    return forward_np(lp_matrix(np.asarray(x)), list(target), blank)


def all_sequences(V, T, blank):
    """Every label sequence of length <= T over the V - 1 labels that are not the blank, shortest first."""
    labels = [c for c in range(V) if c != blank]
    return [list(seq) for n in range(T + 1) for seq in itertools.product(labels, repeat=n)]


# (V, T, hypotheses, of them without an alignment): an utterance of standard-normal float64 logits -- no entry comes near
# the clip at ln 1e-15 -- scored with every label sequence at once. The probabilities of all sequences sum to 1.
NORMALISATION = ((3, 4, 31, 16), (4, 5, 364, 216), (3, 7, 255, 188))


def normalisation_input(V, T):
    return np.random.default_rng(1000 * V + T).standard_normal((T, V))


def neg_inf_case():
    """(x, target): float64 logits [25, 29] that hold -inf at target labels in some frames (and at the blank in one): the
    emissions there take the floor ln 1e-15, and the score stays finite."""
    rng = np.random.default_rng(77)
    target = random_target(rng, 8, 29, doubled=1)
    x = random_logits(rng, 25, 29)
    for t in range(0, 25, 3):
        x[t, target[(t // 3) % len(target)]] = -np.inf
    x[4, 0] = -np.inf
    return x, target


__all__ = ["SCORE_TOL", "SINGLE_PATH", "WAVE_MAX_LABELS", "NORMALISATION", "forward_np", "yardstick", "all_sequences",
           "normalisation_input", "neg_inf_case", "case_input", "feasible", "shape_cases", "random_logits", "random_target"]
