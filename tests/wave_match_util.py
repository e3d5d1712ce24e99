"""TEST INFRASTRUCTURE: inputs whose candidates merge in most frames (the wave kernel's hash match and group fold at
work, which real posteriors leave idle in ~98 % of their frames), their oracle beams -- computed once per session -- and
the strict comparison of tests/test_wave_match.py and tests/test_gpu_wave_match.py."""
import functools

import numpy as np

import synth
from oracle.ctc_oracle import build_oracle
from pyctcdecode_amd.alphabet import Alphabet

TINY_LABELS = ["", "a", "b", " "]  # V = 4: blank, two letters, space -- almost every candidate meets its text's other spellings
N_UTTS = 3

# name -> (labels, frames, decode arguments)
CASES = {
    "tiny20": (TINY_LABELS, 30, {"beam_width": 20}),
    "tiny64": (TINY_LABELS, 30, {"beam_width": 64}),
    # no score prune: more than 64 live beams, a label's candidates are two half passes matched together (pass_big);
    # about a quarter of its frames merge something, so both sides of the pass's "nobody joined anybody" test are taken
    "wide100": (synth.LIBRI_LABELS, 40, {"beam_width": 100, "beam_prune_logp": -1e9}),
}


@functools.lru_cache(maxsize=None)
def inputs(name):
    """N_UTTS utterances [T, V] float64"""
    labels, T, _ = CASES[name]
    V = len(labels) if "" in labels else len(labels) + 1
    rng = np.random.default_rng(20261020 + sorted(CASES).index(name))
    scale = 0.05 if labels is TINY_LABELS else 1.0  # (near-flat / N(0, 1) logits)
    xs = [rng.standard_normal((T, V)) * scale for _ in range(N_UTTS)]
    for x in xs:
        x.setflags(write=False)
    return xs


@functools.lru_cache(maxsize=None)
def expected(name):
    """per utterance: the oracle's beams [(text, [[word, start, end]], logit, lm)]"""
    labels, _, kw = CASES[name]
    alpha = Alphabet.build_alphabet(labels)
    orc = build_oracle(alpha.labels, alpha.is_bpe)
    out = []
    for x in inputs(name):
        with np.errstate(all="ignore"):
            beams = orc.decode_beams(np.array(x), **kw)
        out.append([(o[0], [[w, int(a), int(b)] for w, (a, b) in o[2]], o[3], o[4]) for o in beams])
    return out


def beams_of(outs):
    return [(o.text, [[w, int(a), int(b)] for w, (a, b) in o.text_frames], o.logit_score, o.lm_score) for o in outs]


def assert_same_beams(got, want, what, tol=1e-9):
    """beam for beam: the same texts and word frames in the same ORDER (no tie window), scores within tol (absolute)"""
    assert len(got) == len(want), "%s: %d beams, expected %d" % (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g[:2] == w[:2], "%s: beam %d is %r, expected %r" % (what, k, g[:2], w[:2])
        assert abs(g[2] - w[2]) <= tol and abs(g[3] - w[3]) <= tol, "%s: beam %d scores %r, expected %r" % (what, k, g[2:], w[2:])
