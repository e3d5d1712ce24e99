"""Shared driver of the streaming goldens: tests/golden/cases_stream.json.gz holds what the UNMODIFIED reference's
get_starting_state / partial_decode_beams returned after EVERY step of every scenario (oracle/make_golden_stream.py writes it;
tests/test_stream_golden.py and tests/test_gpu_stream_golden.py replay it). Only expectations are stored: the inputs come
from synth (or inputs.npz for the toy scenario) and are checked against the sha256 the generator took of them.

The generator imports this module for the scenarios' inputs and chunks, so that both sides cut the very same arrays: nothing
here may import the package or the oracle at module level.
"""
import gzip
import hashlib
import json
import math
import os
import warnings

import numpy as np

import synth
from tests.golden_util import GOLD, LM_DIR, TOY_ARPA, check_beams

PATH = os.path.join(GOLD, "cases_stream.json.gz")
LM_SPEC = {"n_words": 300, "n_sent": 400, "order": 4, "seed": 2}
_LM = None


def lm():
    global _LM
    if _LM is None:
        _LM = synth.SynthLM(LM_DIR, LM_SPEC["n_words"], LM_SPEC["n_sent"], order=LM_SPEC["order"], seed=LM_SPEC["seed"])
    return _LM


def labels_of(key, fixture=None):
    """labels key -> (labels, is_bpe). `toy` is the reference's SAMPLE_LABELS, a list of names kept in the fixture."""
    if key == "libri":
        return list(synth.LIBRI_LABELS), False
    if key == "bpe255":
        return synth.make_bpe_vocab(lm().words, size=255), True
    if key == "toy":
        return list(fixture["label_sets"]["toy"]), False
    raise KeyError(key)


def lm_path_of(spec):
    if spec is None:
        return None
    if spec == "toy":
        return TOY_ARPA
    assert spec == LM_SPEC, spec
    return lm().path


def make_input(inp, labels, is_bpe):
    """The whole utterance of a stream as the generator made it (float32 from synth, float64 for the toy matrix)."""
    if inp["kind"] == "npz":
        return np.load(os.path.join(GOLD, inp["file"]))[inp["key"]]
    if inp["kind"] == "d_flat":
        return synth.d_flat(inp["config"], inp["utt"], inp["T"], inp["V"])
    assert inp["kind"] == "d_words", inp
    return synth.d_words(inp["config"], inp["utt"], inp["T"], labels, is_bpe, lm().words, lm().sentences, len(labels),
                         boost=inp["boost"])


def sha256_of(x):
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()


def checked_input(inp, labels, is_bpe):
    x = make_input(inp, labels, is_bpe)
    assert sha256_of(x) == inp["sha256"], "input %r is not the array the golden was generated from" % (inp,)
    return x


def chunk_of(x, step):
    """Rows start:stop of the utterance in the step's dtype; as_probs: their softmax, so that the `probabilities or logits?`
    sniff of that chunk alone says probabilities. (Scalar libm calls in a fixed order: numpy's vector exp differs between
    hosts in the last bit, and generator and tests must feed the same bits.)"""
    c = np.ascontiguousarray(x[step["start"]:step["stop"]].astype(step["dtype"]))
    if not step["as_probs"]:
        return c
    out = np.empty(c.shape, dtype=np.float64)
    for t in range(c.shape[0]):
        row = [float(v) for v in c[t]]
        m = max(row)
        e = [math.exp(v - m) for v in row]
        s = 0.0
        for v in e:
            s += v
        out[t] = [v / s for v in e]
    return out.astype(step["dtype"])


def scorer_key(step):
    return None if step["hotwords"] is None else (tuple(step["hotwords"]), float(step["hotword_weight"]))


def scorer_changes(steps, k):
    """Does step k score with another hot-word set than step k-1 did? (where the refreshed expectation refreshes its memos)"""
    return k > 0 and scorer_key(steps[k]) != scorer_key(steps[k - 1])


def load():
    with gzip.open(PATH, "rt", encoding="utf-8") as f:
        return json.load(f)


FIXTURE = load() if os.path.exists(PATH) else None


def scenarios(kind="stream"):
    return [s for s in FIXTURE["scenarios"] if s["kind"] == kind]


# ---- what is compared: all eight LMBeam fields, through tests.golden_util.check_beams ------------------------------------------
def _ident(text, next_word, partial_word, last_char):
    return "%s|%s|%s|%r" % (text, next_word, partial_word, last_char)


def lm_beams(beams):
    """package / reference LMBeams -> check_beams' `got`: text, next_word, partial_word and last_char make the identity string,
    the partial frames ride at the end of the frame list."""
    return [(_ident(b.text, b.next_word, b.partial_word, b.last_char),
             [(str(k), (int(f[0]), int(f[1]))) for k, f in enumerate(b.text_frames)]
             + [("p", (int(b.partial_frames[0]), int(b.partial_frames[1])))], float(b.logit_score), float(b.lm_score))
            for b in beams]


def oracle_beams(obeams):
    """oracle OBeams (next_word is always folded into the text between calls) -> the same shape"""
    return [(_ident(o.text, "", o.partial, o.last), [(str(k), (int(f[0]), int(f[1]))) for k, f in enumerate(o.tframes)]
             + [("p", (int(o.pframes[0]), int(o.pframes[1])))], float(o.logit), float(o.lm)) for o in obeams]


def golden_beams(stored):
    """stored beams of one step -> check_beams' `expected`"""
    return [{"text": _ident(e["text"], e["next_word"], e["partial_word"], e["last_char"]),
             "frames": [[str(k), int(f[0]), int(f[1])] for k, f in enumerate(e["text_frames"])]
             + [["p", int(e["partial_frames"][0]), int(e["partial_frames"][1])]], "logit": e["logit"], "lm": e["lm"]}
            for e in stored]


def check_steps(got_steps, stream, which="expected", what="", **tol):
    """Every step that was read against the golden of that step. got_steps[k] is None only for a step the plan leaves unread."""
    exp_steps = stream[which]
    assert len(got_steps) == len(exp_steps)
    n = 0
    for k, (got, exp) in enumerate(zip(got_steps, exp_steps)):
        if got is None:
            continue
        check_beams(got, golden_beams(exp), what="%s step %d" % (what, k), **tol)
        n += 1
    return n


# ---- replaying a plan ----------------------------------------------------------------------------------------------------------
def _edit(beams, edit):
    return beams if edit is None else beams[:edit["keep_best"]]


def run_scenario(build, to_input, scenario, batched=False, read_step=None):
    """Replay a scenario's plan against the package. build: build_ctcdecoder; to_input: chunk -> what is fed (host array or
    device tensor). Returns, per stream, the per-step beam lists as check_beams takes them.

    A step whose plan says `read` is looked at (and the list handed back as it is); an unread one stays on the device and gives
    None -- unless read_step names it: the unread scenario is replayed once per step, looking at that step alone, so that every
    step is compared while everything before it took the unread route.
    batched: one partial_decode_beams_batch call per step for all streams; else the streams run one after another."""
    from pyctcdecode_amd.language_model import HotwordScorer

    fx = FIXTURE
    labels, is_bpe = labels_of(scenario["labels"], fx)
    dec = build(labels, lm_path_of(scenario["lm"]), scenario["unigrams"])
    streams = scenario["streams"]
    xs = [checked_input(s["input"], labels, is_bpe) for s in streams]
    kw = dict(scenario["decode"])

    def scorer(step):
        return None if step["hotwords"] is None else HotwordScorer.build_scorer(step["hotwords"], weight=step["hotword_weight"])

    def start(stream):
        beams, c1, c2 = dec.get_starting_state()
        seed = stream.get("seed_state")
        if seed is not None:
            lx = checked_input(seed["input"], labels, is_bpe)
            first = dec.decode_beams(lx.astype(seed["dtype"]), **seed["decode"])
            state = first[0].last_lm_state
            model = dec._language_model._kenlm_model
            assert first[0].text == seed["text"]
            assert [model.word(i) for i in state.state.words] == seed["state"]["words"]
            assert [float(np.float32(b)) for b in state.state.backoff] == seed["state"]["backoff"]
            c1.clear()
            c1[("", False)] = (0.0, 0.0, state)
        return beams, c1, c2

    def looked_at(step, k):
        return step["read"] or step["is_end"] or k == read_step

    out = [[] for _ in streams]
    if batched:
        states = [start(s) for s in streams]
        beams = [s[0] for s in states]
        for k in range(len(streams[0]["steps"])):
            steps = [s["steps"][k] for s in streams]
            s0 = steps[0]
            assert all((st["force_next_word"], st["is_end"], scorer_key(st)) == (s0["force_next_word"], s0["is_end"], scorer_key(s0))
                       for st in steps)
            beams = dec.partial_decode_beams_batch(
                [to_input(chunk_of(x, st)) for x, st in zip(xs, steps)], [s[1] for s in states], [s[2] for s in states], beams,
                [st["start"] for st in steps], hotword_scorer=scorer(s0), force_next_word=s0["force_next_word"],
                is_end=s0["is_end"], **kw)
            for u, st in enumerate(steps):
                out[u].append(lm_beams(beams[u]) if looked_at(st, k) else None)
            beams = [_edit(b, st["edit"]) for b, st in zip(beams, steps)]
        return out
    for u, (stream, x) in enumerate(zip(streams, xs)):
        beams, c1, c2 = start(stream)
        for k, st in enumerate(stream["steps"]):
            beams = dec.partial_decode_beams(to_input(chunk_of(x, st)), c1, c2, beams, st["start"], hotword_scorer=scorer(st),
                                             force_next_word=st["force_next_word"], is_end=st["is_end"], **kw)
            out[u].append(lm_beams(beams) if looked_at(st, k) else None)
            beams = _edit(beams, st["edit"])
    return out


def run_oracle(scenario, refresh):
    """The same plan on oracle/ctc_oracle.py. refresh: the caller refreshes the stream's memos (OracleState.refresh_memos) at every
    step whose hot-word set differs from the previous step's -- the package's contract; without it the oracle keeps the old
    set's memoised bonuses like the reference (`expected_stale`)."""
    from oracle.ctc_oracle import build_oracle
    from pyctcdecode_amd.alphabet import Alphabet

    labels, _ = labels_of(scenario["labels"], FIXTURE)
    alpha = Alphabet.build_alphabet(labels)
    orc = build_oracle(alpha.labels, alpha.is_bpe, lm_path_of(scenario["lm"]), scenario["unigrams"])
    kw = dict(scenario["decode"])
    out = []
    for stream in scenario["streams"]:
        x = checked_input(stream["input"], labels, alpha.is_bpe)
        seed = stream.get("seed_state")
        state = None
        if seed is not None:
            lx = checked_input(seed["input"], labels, alpha.is_bpe)
            with np.errstate(all="ignore"):
                first = orc.decode_beams(lx.astype(seed["dtype"]), **seed["decode"])
            assert first[0][0] == seed["text"]
            state = first[0][1]
        st = orc.get_starting_state(state)
        got = []
        for k, step in enumerate(stream["steps"]):
            if refresh and scorer_changes(stream["steps"], k):
                st.refresh_memos(step["hotwords"], step["hotword_weight"])
            with np.errstate(all="ignore"), warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)  # (numpy on the mean of an empty chunk's row sums)
                ob = orc.partial_decode_beams(chunk_of(x, step), st, step["start"], hotwords=step["hotwords"],
                                              hotword_weight=step["hotword_weight"], force_next_word=step["force_next_word"],
                                              is_end=step["is_end"], **kw)
            got.append(oracle_beams(ob))
            if step["edit"] is not None:
                st.beams = st.beams[:step["edit"]["keep_best"]]
        out.append(got)
    return out
