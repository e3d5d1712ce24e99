"""Beam search at every beam-table size edge (shared by tests/test_beam_widths.py, simulator, and
tests/test_gpu_beam_widths.py, HIP build).

The beam stage is compiled once per beam-table capacity and the capacity is picked from beam_width at launch: the wave
kernel's tables hold 64, 100 or 128 beams (beam_wave.h: wave_bucket; wider decodes go to the workgroup kernel), the workgroup
kernel's 32, 64, 128 or 256 (beam_core.h: beam_bucket), at 256 or 512 threads and candidate chunks of 512 or 1024
(group_cand). WIDTHS sits on both sides of every border of both rules, and the inputs keep the beam list FULL, so that the cut
behind the beam_width-th beam -- where a table one record short, or a selection that mishandles rank B-1 or B, shows -- is
taken in most frames:

  flat   synth.d_flat(2, 5, 48, 29), 29 character labels, no LM, default arguments: 29 survivors a frame.
  words  synth.d_words(2, 5, 60, ..., boost=2.0) with the suite's 4-gram, six hot words (two of them out of vocabulary),
         beam_prune_logp=-25 and, at the odd widths, prune_history.

Both are float64: every prune route is the fp64 one and the fp64 bounds of tests/test_gpu_parity.py (TOL) apply.

The fullness condition is asserted on the oracle alone (check_fullness), stepped one frame at a time: the live list holds
exactly beam_width beams after at least half of the frames -- `flat` at every width, `words` at every width up to 128; `words`
at 129, 255 and 256 holds at least 100 live beams after at least half of the frames. What the oracle gives at these seeds:

  flat   exactly beam_width live beams after 48 of 48 frames at widths 1 and 2, after 47 of 48 at every other width (frame 0
         has 29 candidates); decode_beams returns beam_width beams at every width.
  words  exactly beam_width after 60 of 60 frames at 1 and 2; after 59 at 31, 32, 33, 63, 64, 65, 100 and 128; after 55 at 99,
         101 and 127. At least 100 live beams after 59 of 60 frames at 129, 255 and 256
         (exactly beam_width after 55, 53 and 58). decode_beams returns 28, 28, 30, 56, 56, 57, 88, 88, 88, 110, 110, 112, 219
         and 220 beams at widths 31 .. 256.
  Either input hands exactly A beams over the cut of every stream pair below.

Width changes in a stream (STREAM_PAIRS): frames 0 .. 23 at width A, the rest at width B with is_end. The second chunk
carries in what the first one kept -- up to A beams, more than beam_width B asks for where A > B -- so either kernel runs on
the table that holds max(beam_width, carried beams) (beam_wave.h: wave_table; backend: the workgroup kernel's shape), and more
than 128 carried beams go to the workgroup kernel whatever B is. 100 -> 64, 64 -> 10 and 33 -> 32 carry more than the
workgroup kernel's table for B holds, 100 -> 64 more than the wave kernel's: `words` 100 -> 64 / 64 -> 10 came back with other
beams than the oracle's while the workgroup table was sized by beam_width alone.
"""
import copy
import functools

import numpy as np

import synth
from oracle.ctc_oracle import build_oracle
from pyctcdecode_amd.alphabet import Alphabet
from tests.golden_util import LM_DIR, check_beams

WIDTHS = (1, 2, 31, 32, 33, 63, 64, 65, 99, 100, 101, 127, 128, 129, 255, 256)
INPUTS = ("flat", "words")
TOL = {"tol": 1e-9, "tie_tol": 1e-9}  # tests/test_gpu_parity.py: TOL, the fp64 bounds
CUT = 24
STREAM_PAIRS = ((128, 101), (100, 64), (64, 10), (256, 128), (200, 256), (33, 32))
WORDS_WIDE_FLOOR = 100  # live beams asked of `words` where beam_width > 128


@functools.lru_cache(maxsize=None)
def lm():
    return synth.SynthLM(LM_DIR, 300, 400, order=4, seed=2)


@functools.lru_cache(maxsize=None)
def logits(name):
    if name == "flat":
        x = synth.d_flat(2, 5, 48, 29)
    else:
        x = synth.d_words(2, 5, 60, synth.LIBRI_LABELS, False, lm().words, lm().sentences, 28, boost=2.0)
    x = x.astype(np.float64)
    x.setflags(write=False)
    return x


def arpa(name):
    return lm().path if name == "words" else None


def decode_kwargs(name, width):
    """decode_beams arguments of a case (the oracle takes the same)."""
    if name == "flat":
        return {"beam_width": width}
    return {"beam_width": width, "hotwords": lm().hotwords(6, 2), "beam_prune_logp": -25.0, "prune_history": bool(width % 2)}


def stream_kwargs(name, width):
    """The same case as arguments of the product's partial_decode_beams (a scorer instead of the word list)."""
    from pyctcdecode_amd.language_model import HotwordScorer

    kw = decode_kwargs(name, width)
    hot = kw.pop("hotwords", None)
    if hot is not None:
        kw["hotword_scorer"] = HotwordScorer.build_scorer(hot, weight=10.0)
    return kw


def build_decoder(name):
    from pyctcdecode_amd import build_ctcdecoder

    return build_ctcdecoder(synth.LIBRI_LABELS, arpa(name))


@functools.lru_cache(maxsize=None)
def oracle(name):
    alpha = Alphabet.build_alphabet(synth.LIBRI_LABELS)
    return build_oracle(alpha.labels, alpha.is_bpe, arpa(name), None)


@functools.lru_cache(maxsize=None)
def expected(name, width):
    """The oracle's decode_beams of a case, once per session (1 .. 3 s at the wide widths)."""
    with np.errstate(all="ignore"):
        out = oracle(name).decode_beams(logits(name), **decode_kwargs(name, width))
    return tuple({"text": o[0], "frames": [[w, int(a), int(b)] for w, (a, b) in o[2]], "logit": o[3], "lm": o[4]} for o in out)


def as_tuples(beams):
    return [(o.text, o.text_frames, o.logit_score, o.lm_score) for o in beams]


def utterances(name):
    x = logits(name)
    return [x, x[:17], x[5:]]


def check_case(dec, name, width, to_input=lambda a: a):
    """decode_beams of one case against the oracle, and decode_beams_batch of three utterances against the single calls."""
    kw = decode_kwargs(name, width)
    what = "%s bw%d" % (name, width)
    got = as_tuples(dec.decode_beams(to_input(logits(name)), **kw))
    try:
        check_beams(got, list(expected(name, width)), what=what, **TOL)
    except AssertionError as e:
        raise AssertionError("%s\n%s: the stepped lists part ways with the oracle's at frame %r"
                             % (e, what, first_parting_frame(dec, name, width, to_input))) from e
    xs = utterances(name)
    batch = dec.decode_beams_batch(None, [to_input(x) for x in xs], **kw)
    assert as_tuples(batch[0]) == got, what + ": batch[0] != the single call"
    for u in (1, 2):
        assert as_tuples(batch[u]) == as_tuples(dec.decode_beams(to_input(xs[u]), **kw)), "%s: batch[%d] != the single call" % (what, u)


# ---- the oracle, one frame at a time ------------------------------------------------------------------------------------
def _oracle_step(orc, st, x, t, kw, is_end=False):
    with np.errstate(all="ignore"):
        return orc.partial_decode_beams(x[t:t + 1], st, t, is_end=is_end, **kw)


@functools.lru_cache(maxsize=None)
def live_counts(name, width):
    """Live beams after every frame of the oracle's search (as tools/fuzz_sim_vs_oracle._parted_at_a_tie steps it)."""
    orc, x, kw = oracle(name), logits(name), decode_kwargs(name, width)
    st = orc.get_starting_state()
    return tuple(len(_oracle_step(orc, st, x, t, kw)) for t in range(x.shape[0]))


def fullness_floor(name, width):
    return WORDS_WIDE_FLOOR if name == "words" and width > 128 else width


def full_frames(name, width):
    floor = fullness_floor(name, width)
    return sum(1 for n in live_counts(name, width) if n >= floor)


def check_fullness(name, width):
    """A condition on the case, not a tolerance on the product: the oracle's own search must sit at the cut."""
    counts = live_counts(name, width)
    assert max(counts) <= width, (name, width, max(counts))
    full = full_frames(name, width)
    assert 2 * full >= len(counts), "%s bw%d: %d live beams or more after %d of %d frames only: %r" % (
        name, width, fullness_floor(name, width), full, len(counts), counts)


def first_parting_frame(dec, name, width, to_input=lambda a: a):
    """Diagnosis of a mismatch: the first frame after which the product's live list (texts and open words, in order) is not
    the oracle's, both stepped one frame at a time; None if they never part."""
    orc, x = oracle(name), logits(name)
    okw, kw = decode_kwargs(name, width), stream_kwargs(name, width)
    beams, c1, c2 = dec.get_starting_state()
    st = orc.get_starting_state()
    T = x.shape[0]
    for t in range(T):
        beams = dec.partial_decode_beams(to_input(x[t:t + 1]), c1, c2, beams, t, is_end=(t == T - 1), **kw)
        ob = _oracle_step(orc, st, x, t, okw, is_end=(t == T - 1))
        if [(b.text, b.partial_word) for b in beams] != [(o.text, o.partial) for o in ob]:
            return t
    return None


# ---- width changes in a stream ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_at_the_cut(name, a):
    """The oracle's stream state behind chunk one (frames 0 .. CUT-1 at width a), computed once; users take a copy."""
    orc, x = oracle(name), logits(name)
    st = orc.get_starting_state()
    with np.errstate(all="ignore"):
        carried = len(orc.partial_decode_beams(x[:CUT], st, 0, **decode_kwargs(name, a)))
    return carried, st


@functools.lru_cache(maxsize=None)
def stream_expected(name, a, b, length=None):
    """The oracle stepped at the same cut: (beams carried over the cut, final beams as check_beams takes them).
    length: frames of chunk two (None: the rest of the input)."""
    orc, x = oracle(name), logits(name)
    carried, st = _oracle_at_the_cut(name, a)
    st = copy.deepcopy(st)
    end = x.shape[0] if length is None else CUT + length
    with np.errstate(all="ignore"):
        out = orc.partial_decode_beams(x[CUT:end], st, CUT, is_end=True, **decode_kwargs(name, b))
    return carried, tuple({"text": o.text, "frames": [[w, int(f[0]), int(f[1])] for w, f in zip(o.text.split(), o.tframes)],
                           "logit": o.logit, "lm": o.lm} for o in out)


# A short chunk two behind a wide chunk one: the first frame advances every carried beam -- far more than beam_width B -- and
# there are no later frames whose share of the node arenas could absorb that. The narrowing pairs above and two steeper ones;
# chunk two of one frame and of three.
SHORT_PAIRS = tuple(p for p in STREAM_PAIRS if p[0] > p[1]) + ((128, 20), (256, 10))
SHORT_LENGTHS = (1, 3)


# last_beam_kernel after chunk two under a forced wave kernel (1: the wave kernel, 2: the workgroup kernel; forced `group`: 2
# throughout): 256 carried beams and beam_width 256 are more than any wave table holds; 100 -> 64 runs on beam_wave<100>.
WAVE_STREAM_KERNEL = {(256, 128): 2, (128, 101): 1, (100, 64): 1, (64, 10): 1, (200, 256): 2, (33, 32): 1}


def check_stream_pair(dec, name, a, b, to_input=lambda a: a, edit=False, length=None):
    """Two chunks at widths a and b against the oracle. edit: hand chunk two a plain copy of the list (the host resolves and
    imports the beams again) instead of the device-resident one. length: frames of chunk two (None: the rest)."""
    x = logits(name)
    end = x.shape[0] if length is None else CUT + length
    beams, c1, c2 = dec.get_starting_state()
    beams = dec.partial_decode_beams(to_input(x[:CUT]), c1, c2, beams, 0, **stream_kwargs(name, a))
    if edit:
        beams = list(beams)
    beams = dec.partial_decode_beams(to_input(x[CUT:end]), c1, c2, beams, CUT, is_end=True, **stream_kwargs(name, b))
    carried, exp = stream_expected(name, a, b, length)
    assert carried == a  # (the cases: the first chunk hands on a full list)
    got = [(o.text, list(zip(o.text.split(), o.text_frames)), o.logit_score, o.lm_score) for o in beams]
    check_beams(got, list(exp), what="%s stream %d->%d%s%s" % (name, a, b, "" if length is None else " x%d" % length,
                                                              " (host import)" if edit else ""), **TOL)
