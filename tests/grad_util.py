"""Transcript gradient (BeamSearchDecoderCTC.gradient / gradient_batch / ctc_loss; DESIGN.md "Transcript gradient"), shared by
the CPU and GPU tests: three yardsticks written from the definition, not from csrc/ctc_align.h, the tolerances, and the checks
every result goes through.

Yardsticks:
  1. grad_np: the numpy forward-backward of tests/posteriors_util.py over lp_matrix, gamma folded by label, then the formula
     (logits: G' - exp(x - lse) M with u from the raw input; probabilities: G / p inside the clip). Every result is held to it.
  2. grad_torch: torch.nn.functional.ctc_loss (CPU, float64, reduction="sum") over clamp(log_softmax(x), ln 1e-15, 0),
     differentiated by autograd. Logits with nothing clipped only: torch's CTC backward returns exp(lp) - G with respect to
     log_probs, which assumes rows that sum to 1 -- on probability-like input it is off by exactly 1 per entry.
  3. grad_recursion: autograd through a hand-written float64 forward recursion in torch (logsumexp over stay / step / skip),
     for probabilities and clipped entries, T <= 60. It assumes nothing about the rows.

Tolerances, from the project's own SCORE_TOL = 1e-9 and GAMMA_TOL = 4e-9: gamma's error is relative to gamma and a row of gamma
sums to 1, so |dG'| <= GAMMA_TOL and |dM| <= GAMMA_TOL, and a softmax entry is at most 1:
  GRAD_TOL = 2 * GAMMA_TOL absolute on every entry of a logits gradient;
  GAMMA_TOL on p * grad of a probability-like utterance (G / p itself is unbounded: up to 1.1e5 in V29_probs);
  F32_ROUND = 2^-24 more for a float32 result (|G'|, |softmax M| and p * |G / p| are at most 1: one rounding each);
  YARDSTICK_TOL = 1e-10 between the yardsticks themselves, p * grad for probabilities (measured: 4.1e-12 at limit_L2047, 6.5e-14 on the clipped cases)."""
import math

import numpy as np

from pyctcdecode_amd.constants import MIN_TOKEN_CLIP_P
from tests.posteriors_util import GAMMA_TOL, SCORE_TOL, fwdbwd_np, states_of
from tests.score_util import neg_inf_case
from tests.token_logp_util import lp_matrix

GRAD_TOL = 2 * GAMMA_TOL
F32_ROUND = 2.0 ** -24
YARDSTICK_TOL = 1e-10
FLOOR = math.log(MIN_TOKEN_CLIP_P)
RECURSION_MAX_T = 60


def looks_like_probs(x):
    """The rule of lp_matrix (the reference's, decoder.py:760), on the raw input in its own dtype."""
    x = np.asarray(x)
    return bool(len(x)) and math.isclose(float(x.sum(axis=1).mean()), 1.0)


def unclipped(x):
    """[T, V] bool: the entries whose emission the clip does not hold (u of the definition), from the raw input."""
    x = np.asarray(x)
    xd = x.astype(np.float64)
    if looks_like_probs(x):
        return (xd >= MIN_TOKEN_CLIP_P) & (xd <= 1.0)
    with np.errstate(invalid="ignore"):
        m = xd.max(axis=1, keepdims=True)
        lse = m + np.log(np.exp(xd - m).sum(axis=1, keepdims=True))
        return xd - lse >= FLOOR


def grad_np(x, target, blank):
    """Yardstick 1 -> (logp, grad [T, V] float64)."""
    x = np.asarray(x)
    xd = x.astype(np.float64)
    T, V = xd.shape
    logp, gamma = fwdbwd_np(lp_matrix(x), list(target), blank)
    ext, _ = states_of(list(target), blank)
    G = np.zeros((T, V))
    for s, k in enumerate(ext.tolist()):
        G[:, k] += gamma[:, s]
    u = unclipped(x)
    if looks_like_probs(x):
        with np.errstate(divide="ignore", invalid="ignore"):
            return logp, np.where(u, G / xd, 0.0)
    m = xd.max(axis=1, keepdims=True)
    lse = m + np.log(np.exp(xd - m).sum(axis=1, keepdims=True))
    Gp = np.where(u, G, 0.0)
    return logp, Gp - np.exp(xd - lse) * Gp.sum(axis=1, keepdims=True)


def grad_torch(x, target, blank):
    """Yardstick 2 -> (logp, grad): logits with nothing clipped."""
    import torch

    xt = torch.tensor(np.asarray(x).astype(np.float64), requires_grad=True)
    T = xt.shape[0]
    lp = torch.clamp(torch.log_softmax(xt, dim=-1), FLOOR, 0.0)
    loss = torch.nn.functional.ctc_loss(lp[:, None, :], torch.tensor([list(target)], dtype=torch.long), torch.tensor([T]),
                                        torch.tensor([len(target)]), blank=blank, reduction="sum", zero_infinity=False)
    loss.backward()
    return -float(loss.detach()), (-xt.grad).numpy()


def grad_recursion(x, target, blank):
    """Yardstick 3 -> (logp, grad): any input, T <= RECURSION_MAX_T. States a path cannot be in hold -1e30, not -inf: exp turns
    it into exactly 0, and logsumexp's derivative stays finite."""
    import torch

    x = np.asarray(x)
    assert len(x) <= RECURSION_MAX_T
    xt = torch.tensor(x.astype(np.float64), requires_grad=True)
    if looks_like_probs(x):
        lp = torch.log(torch.clamp(xt, MIN_TOKEN_CLIP_P, 1.0))
    else:
        lp = torch.clamp(xt - torch.logsumexp(xt, dim=-1, keepdim=True), FLOOR, 0.0)
    ext, can_skip = states_of(list(target), blank)
    S, NEG = len(ext), -1e30
    ext_t, skip_t = torch.tensor(ext), torch.tensor(can_skip)
    start = torch.zeros(S, dtype=torch.bool)
    start[:2] = True
    alpha = torch.where(start, lp[0, ext_t], torch.full((S,), NEG, dtype=torch.float64))
    neg1, neg2 = torch.full((1,), NEG, dtype=torch.float64), torch.full((2,), NEG, dtype=torch.float64)
    for t in range(1, len(x)):
        step = torch.cat([neg1, alpha[:-1]])
        skip = torch.where(skip_t, torch.cat([neg2, alpha[:-2]])[:S], torch.full((S,), NEG, dtype=torch.float64))
        alpha = torch.logsumexp(torch.stack([alpha, step, skip]), dim=0) + lp[t, ext_t]
    logp = torch.logsumexp(alpha[-2:], dim=0)
    logp.backward()
    return float(logp.detach()), xt.grad.numpy()


def clipped_target_case():
    """(x, target): float64 logits [30, 12] whose target labels are themselves clipped: label 3 sits 45 below the others in
    every frame (30 entries at the floor) and label 5 at -60 in frame 7 (one more). There a target entry's gradient is
    -softmax * M alone."""
    x = 3.0 * np.random.default_rng(31).standard_normal((30, 12))
    x[:, 3] -= 45.0
    x[7, 5] = -60.0
    return x, [3, 5, 3, 3, 7]


def check_gradient(got, want, x, target, what, on_device=False):
    """One TranscriptGradient against yardstick 1's (logp, grad): type, shape, logp and every entry; prints the worst gaps.
    Returns grad as a float64 numpy array."""
    x = np.asarray(x)
    want_logp, want_grad = want
    wide = x.dtype == np.float64
    assert got.tokens == list(target)
    if on_device:
        import torch

        assert isinstance(got.grad, torch.Tensor) and got.grad.is_cuda, what
        assert got.grad.dtype == (torch.float64 if wide else torch.float32), (what, got.grad.dtype)
        grad = got.grad.double().cpu().numpy()
    else:
        assert isinstance(got.grad, np.ndarray) and got.grad.dtype == (np.float64 if wide else np.float32), (what, got.grad.dtype)
        grad = got.grad.astype(np.float64)
    assert tuple(got.grad.shape) == x.shape, (what, tuple(got.grad.shape))
    if len(x) == 0:
        assert got.logp == 0.0
        return grad
    assert np.isfinite(grad).all(), what
    gap_logp = abs(got.logp - want_logp)
    probs = looks_like_probs(x)
    scale = x.astype(np.float64) if probs else 1.0
    gap = float(np.abs(scale * (grad - want_grad)).max())
    tol = (GAMMA_TOL if probs else GRAD_TOL) + (0.0 if wide else F32_ROUND)
    print("%s: logp %.12f, numpy %+.1e; %s %.1e (bound %.1e), largest |grad| %.3g"
          % (what, got.logp, gap_logp, "p * grad" if probs else "grad", gap, tol, float(np.abs(grad).max())))
    assert gap_logp <= SCORE_TOL, (what, got.logp, want_logp)
    assert gap <= tol, (what, gap, tol)
    return grad


def check_rows(grad, x, target, blank, what):
    """The row properties of a logits gradient with nothing clipped: rows sum to 0, entries off the target and the blank are
    not positive, nothing exceeds 1."""
    assert not looks_like_probs(x) and unclipped(x).all(), what
    tol = GRAD_TOL + (0.0 if np.asarray(x).dtype == np.float64 else F32_ROUND)
    rows = float(np.abs(grad.sum(axis=1)).max())
    off = np.ones(grad.shape[1], dtype=bool)
    off[[blank] + list(target)] = False
    top = float(grad[:, off].max()) if off.any() else 0.0
    print("%s: rows sum to %.1e, off-target maximum %.1e, largest entry %.6f" % (what, rows, top, float(np.abs(grad).max())))
    assert rows <= tol, (what, rows)
    assert top <= 0.0, (what, top)
    assert float(np.abs(grad).max()) <= 1.0 + tol, what


def same_bits(a, b):
    """Two TranscriptGradients, float for float (numpy arrays or torch tensors)."""
    ga = a.grad if isinstance(a.grad, np.ndarray) else a.grad.cpu().numpy()
    gb = b.grad if isinstance(b.grad, np.ndarray) else b.grad.cpu().numpy()
    return (a.text == b.text and a.tokens == b.tokens and a.logp == b.logp and ga.dtype == gb.dtype and ga.shape == gb.shape
            and np.array_equal(ga.view(np.uint8), gb.view(np.uint8)))


__all__ = ["GRAD_TOL", "GAMMA_TOL", "SCORE_TOL", "F32_ROUND", "YARDSTICK_TOL", "grad_np", "grad_torch", "grad_recursion",
           "unclipped", "looks_like_probs", "clipped_target_case", "neg_inf_case", "check_gradient", "check_rows", "same_bits"]
