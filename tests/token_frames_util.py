"""Checks of the token-frame contract (decode_beams(..., token_frames=True), DESIGN.md "Token frames"), shared by the CPU and
GPU tests: every beam's token_frames against its own text_frames (property 1), their order (2) and the frame's token prune (3)."""
import math

import numpy as np

from pyctcdecode_amd.constants import MIN_TOKEN_CLIP_P

BPE_TOKEN = "▁"


def log_probs(x):
    """The [T, V] float64 matrix the decoder's frame prune looks at (decoder.py:759-765: rows whose mean sum is 1 are
    probabilities)."""
    x = np.asarray(x, dtype=np.float64)
    if len(x) and math.isclose(float(x.sum(axis=1).mean()), 1.0):
        return np.log(np.clip(x, MIN_TOKEN_CLIP_P, 1))
    m = x.max(axis=1, keepdims=True)
    lse = m + np.log(np.exp(x - m).sum(axis=1, keepdims=True))
    return np.clip(x - lse, np.log(MIN_TOKEN_CLIP_P), 0)


def clean(label, is_bpe):
    if not is_bpe:
        return label
    if label[:1] == BPE_TOKEN:
        label = label[1:]
    if label[-1:] == BPE_TOKEN:
        label = label[:-1]
    return label


def check_tokens(text_frames, tokens, labels, is_bpe, lp=None, token_min_logp=-5.0, what=""):
    """tokens: [(label, (start, end))]; lp: the [T, V] log-probabilities for property 3 (None: skip it)."""
    n = len(tokens)
    for k, (lab, (s, e)) in enumerate(tokens):
        assert lab in labels and lab != "", (what, k, lab)
        if not is_bpe:
            assert lab != " ", (what, "a space label is not a token", k)
        assert 0 <= s < e, (what, k, s, e)
        if k + 1 < n:
            lab2, (s2, _e2) = tokens[k + 1]
            assert e <= s2, (what, k, e, s2)
            if lab2 == lab:
                assert e < s2, (what, "equal labels without a gap", k)
    # 1: each word is a run of consecutive tokens; tokens outside the runs have empty cleaned labels
    i = 0
    for word, (ws, we) in text_frames:
        j = i
        while j < n and clean(tokens[j][0], is_bpe) == "":
            j += 1
        opener = [k for k in range(i, min(j, n - 1) + 1) if tokens[k][1][0] == ws]
        assert len(opener) == 1, (what, "no token starts word", word, ws, tokens[i : j + 1])
        acc, m = "", j
        while m < n and len(acc) < len(word):
            acc += clean(tokens[m][0], is_bpe)
            m += 1
        assert acc == word, (what, word, acc, tokens[j:m])
        assert tokens[m - 1][1][1] == we, (what, word, we, tokens[m - 1])
        i = m
    assert all(clean(t[0], is_bpe) == "" for t in tokens[i:]), (what, "tokens after the last word", tokens[i:])
    # 3: the label survived the token prune at its first and its last frame
    if lp is not None:
        index = {lab: c for c, lab in enumerate(labels)}
        for lab, (s, e) in tokens:
            c = index[lab]
            for f in (s, e - 1):
                row = lp[f]
                assert row[c] >= token_min_logp or c == int(np.argmax(row)), (what, lab, s, e, f, row[c])


def check_beams(beams, labels, is_bpe, lp=None, token_min_logp=-5.0, what=""):
    for k, b in enumerate(beams):
        check_tokens(list(b.text_frames), b.token_frames, labels, is_bpe, lp, token_min_logp, "%s beam %d" % (what, k))
