"""Checks of the token and word confidences (decode_beams(..., confidence=...), DESIGN.md "Token confidences"), shared by the
CPU and GPU tests: every token_logp against the numpy fold of the frame prune's own matrix, every word_logp against its tokens."""
import math

import numpy as np

from pyctcdecode_amd.constants import MIN_TOKEN_CLIP_P

FOLDS = ("mean", "min", "max")
# float64 input: the device's float64 log-softmax is the reference's; log_probs() restates it in numpy with a handful of float64
# roundings on magnitudes <= 34.6 (< 1e-13), and a sequential float64 sum of at most 1e4 such terms stays far below 1e-9. A wrong
# frame or label is orders of magnitude outside it.
TOL_F64 = 1e-9
# float32 / float16 / bfloat16 input against the float64 matrix of the same (up-cast) values: the project's documented tolerance
# class for those dtypes (README, "bound 1e-4").
TOL_LOW = 1e-4
LOGP_FLOOR = math.log(MIN_TOKEN_CLIP_P)


def lp_matrix(x):
    """log_probs() of tests/token_frames_util.py for an input of any dtype: the probability test is the reference's, in the
    input's own dtype (decoder.py:760; float32 rows that sum to 1 in float32 do not in float64), the matrix itself the float64
    one of the up-cast values."""
    x = np.asarray(x)
    xd = x.astype(np.float64)
    if len(x) and math.isclose(float(x.sum(axis=1).mean()), 1.0):
        return np.log(np.clip(xd, MIN_TOKEN_CLIP_P, 1))
    m = xd.max(axis=1, keepdims=True)
    lse = m + np.log(np.exp(xd - m).sum(axis=1, keepdims=True))
    return np.clip(xd - lse, np.log(MIN_TOKEN_CLIP_P), 0)


def tol_of(dtype):
    return TOL_F64 if np.dtype(dtype) == np.float64 else TOL_LOW


def fold_of(column, fold):
    """The fold of the float64 log-probabilities of one token's frames, as the definition states it."""
    if fold == "mean":
        acc = 0.0
        for v in column.tolist():  # (ascending frame order, float64)
            acc += v
        return acc / len(column)
    return float(column.min()) if fold == "min" else float(column.max())


def check_token_logp(tokens, token_logp, labels, lp, fold, tol, what=""):
    """tokens: [(label, (start, end))]; token_logp: parallel floats; lp: the [T, V] float64 matrix of log_probs()."""
    assert len(token_logp) == len(tokens), (what, len(token_logp), len(tokens))
    index = {lab: c for c, lab in enumerate(labels)}
    for k, ((lab, (s, e)), got) in enumerate(zip(tokens, token_logp)):
        want = fold_of(lp[s:e, index[lab]], fold)
        assert abs(got - want) <= tol, (what, k, lab, s, e, got, want, got - want)
        assert LOGP_FLOOR <= got <= 0.0, (what, k, got)


def check_logp(beams, labels, lp, fold, tol, what=""):
    n = 0
    for b_i, b in enumerate(beams):
        w = "%s beam %d" % (what, b_i)
        assert len(b.token_logp) == len(b.token_frames), w
        assert len(b.word_logp) == len(b.text_frames), w
        check_token_logp(b.token_frames, b.token_logp, labels, lp, fold, tol, w)
        for (word, (ws, we)), got in zip(b.text_frames, b.word_logp):
            run = [v for (_lab, (s, e)), v in zip(b.token_frames, b.token_logp) if ws <= s and e <= we]
            assert run and got == min(run), (w, word, ws, we, got, run)
            assert LOGP_FLOOR <= got <= 0.0, (w, word, got)
        n += len(b.token_logp)
    return n


def same_but_for_confidence(conf_beams, token_beams):
    """Text, frames, scores, order and token frames of a confidence call equal the token_frames=True call's."""
    key = lambda b: (b.text, list(b.text_frames), b.logit_score, b.lm_score, b.token_frames)  # noqa: E731
    assert [key(b) for b in conf_beams] == [key(b) for b in token_beams]
