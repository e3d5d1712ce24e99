"""ORACLE PINNING OF THE STREAMING CALLS (this container only): drive the UNMODIFIED reference's get_starting_state /
partial_decode_beams (/root/reference, imported through oracle/refshim/) through chunked scenarios -- one-frame and empty chunks,
a chunk of probabilities among logits, float32 chunks, force_next_word in mid-stream, hot words kept / changed / dropped
between chunks, an edited beam list, a memo seeded with another segment's LM state, streams out of phase -- and store EVERY
LMBeam it returned after EVERY step, plus BASELINE configs[0] taken literally (29 labels, no LM, beam 10, T=200).

    python oracle/make_golden_stream.py        (~1 minute)

Output (committed): tests/golden/cases_stream.json.gz. Only plans and expectations are stored; the inputs are seeded
(tests/stream_golden_util.make_input) and the fixture holds a sha256 of each.

Hot words that change in mid-stream: the reference memoises (lm + hot-word bonus, raw lm, state) per text in cached_lm_scores
and one score per partial word in cached_p_lm_scores, so texts and partial words met under the old scorer keep ITS bonus
(`expected_stale`). The package scores everything against the new set, which equals the reference whose caller -- here: this
script -- recomputes the totals of cached_lm_scores with the new scorer and clears cached_p_lm_scores at the change
(`expected`). Both are stored, and they must differ, else the scenario proves nothing.
"""
import gzip
import io
import json
import os
import sys

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(HERE, "refshim"), "/root/reference", ROOT]
os.chdir("/tmp")

import logging  # noqa: E402
import warnings  # noqa: E402

import numpy as np  # noqa: E402

logging.disable(logging.CRITICAL)
warnings.simplefilter("ignore")

from pyctcdecode import build_ctcdecoder  # noqa: E402  (the reference)
from pyctcdecode.language_model import HotwordScorer  # noqa: E402
import pyctcdecode.tests.test_decoder as rt  # noqa: E402

from tests import stream_golden_util as U  # noqa: E402

LM = U.lm()
HOT_A, W_A = LM.hotwords(4, 1), 8.0
HOT_B, W_B = LM.hotwords(3, 2), 3.0
A = (HOT_A, W_A)
B = (HOT_B, W_B)
PLAN_P = [0, 30, 31, 60, 75, 90]
LABEL_SETS = {"toy": list(rt.SAMPLE_LABELS)}
FIXTURE_VIEW = {"label_sets": LABEL_SETS}


def steps_of(cuts, hot=None, force=(), probs=(), dtype="float64", read=True, edit=None):
    """cuts -> steps; hot: one (words, weight) / None for all steps or a list per step; force / probs: step indices;
    edit: {step index: edit}. The last step is the stream's end."""
    n = len(cuts) - 1
    hots = hot if isinstance(hot, list) else [hot] * n
    assert len(hots) == n
    return [{"start": cuts[k], "stop": cuts[k + 1], "as_probs": k in probs, "dtype": dtype,
             "hotwords": None if hots[k] is None else list(hots[k][0]), "hotword_weight": None if hots[k] is None else hots[k][1],
             "force_next_word": k in force, "is_end": k == n - 1, "read": bool(read), "edit": (edit or {}).get(k)}
            for k in range(n)]


def words_input(labels_key, seed, T):
    labels, is_bpe = U.labels_of(labels_key, FIXTURE_VIEW)
    inp = {"kind": "d_words", "config": 3, "utt": seed, "T": T, "boost": 5.0}
    inp["sha256"] = U.sha256_of(U.make_input(inp, labels, is_bpe))
    return inp


def beams_json(beams):
    return [{"text": b.text, "next_word": b.next_word, "partial_word": b.partial_word, "last_char": b.last_char,
             "text_frames": [[int(f[0]), int(f[1])] for f in b.text_frames],
             "partial_frames": [int(b.partial_frames[0]), int(b.partial_frames[1])],
             "logit": float(b.logit_score), "lm": float(b.lm_score)} for b in beams]


def state_to_json(ref_dec, st):
    model = ref_dec._language_model._kenlm_model
    return {"words": [model.words[i] for i in st.state.words], "backoff": [float(b) for b in st.state.backoff]}


def run_reference(dec, labels, is_bpe, stream, decode, refresh):
    """One stream through the reference, as its caller would: the returned list goes back in (edited where the plan says so).
    refresh: at a step whose scorer differs from the previous step's, recompute the memoised totals and drop the partial-word
    scores."""
    x = U.make_input(stream["input"], labels, is_bpe)
    beams, c1, c2 = dec.get_starting_state()
    seed = stream.get("seed_state")
    if seed is not None:
        lx = U.make_input(seed["input"], labels, is_bpe).astype(seed["dtype"])
        first = dec.decode_beams(lx, **seed["decode"])
        seed["text"] = first[0].text
        seed["state"] = state_to_json(dec, first[0].last_lm_state)
        c1.clear()
        c1[("", False)] = (0.0, 0.0, first[0].last_lm_state)
    out = []
    for k, step in enumerate(stream["steps"]):
        scorer = None if step["hotwords"] is None else HotwordScorer.build_scorer(step["hotwords"], weight=step["hotword_weight"])
        if refresh and U.scorer_changes(stream["steps"], k):
            new = scorer or HotwordScorer.build_scorer([], weight=0.0)
            for key, (_, raw, state) in list(c1.items()):
                c1[key] = (raw + new.score(key[0]), raw, state)
            c2.clear()
        with np.errstate(all="ignore"):
            beams = dec.partial_decode_beams(U.chunk_of(x, step), c1, c2, beams, step["start"], hotword_scorer=scorer,
                                             force_next_word=step["force_next_word"], is_end=step["is_end"], **decode)
        out.append(beams_json(beams))
        if step["edit"] is not None:
            beams = beams[:step["edit"]["keep_best"]]
    return out


SCENARIOS = []


def add(name, labels_key, lm, decode, streams, unigrams=None, two_expectations=False):
    labels, is_bpe = U.labels_of(labels_key, FIXTURE_VIEW)
    dec = build_ctcdecoder(list(labels), U.lm_path_of(lm), unigrams)
    for s in streams:
        s["expected"] = run_reference(dec, labels, is_bpe, s, decode, refresh=True)  # (no scorer change: nothing to refresh)
        if two_expectations:
            s["expected_stale"] = run_reference(dec, labels, is_bpe, s, decode, refresh=False)
            assert s["expected"] != s["expected_stale"], "%s: refreshed == stale, the scenario proves nothing" % name
        else:
            assert not any(U.scorer_changes(s["steps"], k) for k in range(len(s["steps"]))), name
        if s.get("seed_state") is not None:  # (the seed has to matter on this input)
            cold = run_reference(dec, labels, is_bpe, {"input": s["input"], "steps": s["steps"]}, decode, refresh=False)
            assert cold != s["expected"], "%s: the seeded stream equals the unseeded one" % name
    dec.cleanup()
    SCENARIOS.append({"name": name, "kind": "stream", "labels": labels_key, "lm": lm, "unigrams": unigrams, "decode": decode,
                      "two_expectations": two_expectations, "streams": streams})
    print(name, [[len(b) for b in s["expected"]] for s in streams], file=sys.stderr)


def one(inp, steps, **extra):
    return [dict({"input": inp, "steps": steps}, **extra)]


def main():
    spec = U.LM_SPEC
    toy_in = {"kind": "npz", "file": "inputs.npz", "key": "x000"}
    toy_x = U.make_input(toy_in, None, False)
    assert np.array_equal(toy_x, np.asarray(rt.TEST_LOGITS)) and toy_x.dtype == np.float64
    toy_in["sha256"] = U.sha256_of(toy_x)
    toy_cuts = [0, 3, 8, int(toy_x.shape[0])]
    add("toy_lm", "toy", "toy", {}, one(dict(toy_in), steps_of(toy_cuts)), unigrams=["bugs", "bunny"])
    add("toy_nolm", "toy", None, {}, one(dict(toy_in), steps_of(toy_cuts)))

    add("char_mixed", "libri", spec, {"beam_width": 40, "prune_history": True},
        one(words_input("libri", 9, 90), steps_of([0, 30, 31, 60, 60, 75, 90], hot=A, probs=(4,))))
    b100 = {"beam_width": 100, "prune_history": True}
    b200 = {"beam_width": 200}
    add("bpe_force_mid", "bpe255", spec, b100, one(words_input("bpe255", 4, 90), steps_of(PLAN_P, force=(2,))))
    add("bpe_force_unread", "bpe255", spec, b100, one(words_input("bpe255", 4, 90), steps_of(PLAN_P, force=(2,), read=False)))
    add("bpe_wide_f32", "bpe255", spec, b200, one(words_input("bpe255", 5, 90), steps_of(PLAN_P, dtype="float32")))
    add("bpe_nolm_hot", "bpe255", None, {"beam_width": 100}, one(words_input("bpe255", 4, 90), steps_of(PLAN_P, hot=A)))
    add("hot_same", "bpe255", spec, b100, one(words_input("bpe255", 4, 90), steps_of(PLAN_P, hot=A)))
    for tag, seed, decode in (("s4_b100", 4, b100), ("s5_b200", 5, b200)):
        add("hot_change_" + tag, "bpe255", spec, decode,
            one(words_input("bpe255", seed, 90), steps_of(PLAN_P, hot=[A, B, B, B, B])), two_expectations=True)
        add("hot_dropped_" + tag, "bpe255", spec, decode,
            one(words_input("bpe255", seed, 90), steps_of(PLAN_P, hot=[A, A, None, None, None])), two_expectations=True)
    add("hot_change_force", "bpe255", spec, b100,
        one(words_input("bpe255", 4, 90), steps_of(PLAN_P, hot=[A, B, B, A, None], force=(2,))), two_expectations=True)
    add("edited", "bpe255", spec, b100,
        one(words_input("bpe255", 4, 90), steps_of(PLAN_P, force=(3,), edit={0: {"keep_best": 7}})))
    add("seeded", "libri", spec, {"beam_width": 40},
        one(words_input("libri", 4, 60), steps_of([0, 25, 60]),
            seed_state={"input": words_input("libri", 3, 60), "dtype": "float64", "decode": {}}))
    phase_cuts = [[0, 1, 40, 40, 70, 96], [0, 33, 34, 35, 90, 96], [0, 20, 48, 64, 65, 96], [0, 5, 6, 50, 96, 96]]
    for tag, key, decode in (("char_b40", "libri", {"beam_width": 40}), ("bpe_b100", "bpe255", {"beam_width": 100}),
                             ("bpe_b200", "bpe255", {"beam_width": 200})):
        add("phases_" + tag, key, spec, decode,
            [{"input": words_input(key, 20 + u, 96), "steps": steps_of(cuts, force=(2,))} for u, cuts in enumerate(phase_cuts)])

    # BASELINE configs[0], literally: 29-character alphabet, no LM, beam 10, one [200, 29] matrix of N(0,1) logits
    inp = {"kind": "d_flat", "config": 0, "utt": 0, "T": 200, "V": 29}
    x = U.make_input(inp, None, False)
    inp["sha256"] = U.sha256_of(x)
    ref = build_ctcdecoder(list(U.labels_of("libri")[0]))
    with np.errstate(all="ignore"):
        text = ref.decode(x, beam_width=10)
        beams = ref.decode_beams(x, beam_width=10)
    SCENARIOS.append({"name": "config0_literal", "kind": "decode", "labels": "libri", "lm": None, "unigrams": None,
                      "decode": {"beam_width": 10}, "input": inp, "dtype": "float32", "text": text,
                      "expected": [{"text": b.text, "frames": [[w, int(f[0]), int(f[1])] for w, f in b.text_frames],
                                    "logit": float(b.logit_score), "lm": float(b.lm_score)} for b in beams]})
    ref.cleanup()
    print("config0_literal", len(beams), repr(text[:40]), file=sys.stderr)

    raw = json.dumps({"label_sets": LABEL_SETS, "lm": spec, "scenarios": SCENARIOS}, ensure_ascii=False,
                     separators=(",", ":")).encode("utf-8")
    buf = io.BytesIO()
    with gzip.GzipFile(filename="", mode="wb", fileobj=buf, compresslevel=9, mtime=0) as f:  # (no name, no time: same bytes)
        f.write(raw)
    with open(U.PATH, "wb") as f:
        f.write(buf.getvalue())
    print("wrote %s: %d scenarios, %d bytes (%d raw)" % (U.PATH, len(SCENARIOS), len(buf.getvalue()), len(raw)), file=sys.stderr)


if __name__ == "__main__":
    main()
