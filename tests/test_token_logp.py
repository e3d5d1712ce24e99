"""Token and word confidences (confidence="mean" | "min" | "max" on decode_beams / decode_beams_batch / decode_batch) on the CPU
simulator of the kernels, which runs the per-token body of csrc/token_logp.h itself: every token of every beam of the committed
reference goldens against the numpy fold of the frame prune's own matrix, a hand-built input whose folds are known by
construction, the array form of decode_batch, time-sliced host ingest, DevicePool and the unchanged defaults. No token is
left out of a check. The HIP build: tests/test_gpu_token_logp.py."""
import json
import math
import os
import pickle

import numpy as np
import pytest

import synth
from tests.golden_util import GOLD, LM_DIR, TOY_ARPA, lm_path, load_cases
from tests.sim_util import sim_library  # noqa: F401
from tests.token_frames_util import log_probs
from tests.token_logp_util import FOLDS, TOL_F64, TOL_LOW, check_logp, check_token_logp, lp_matrix, same_but_for_confidence, tol_of

CASES, INPUTS = load_cases()
with open(os.path.join(GOLD, "cases_probs.json")) as _f:
    PROB_CASES = json.load(_f)["cases"]
PROB_INPUTS = np.load(os.path.join(GOLD, "inputs_probs.npz"))
PROB_LABELS = [" ", "b", "g", "n", "s", "u", "y", ""]
LM = synth.SynthLM(LM_DIR, 300, 400, order=4, seed=2)

CHARS = ["", " ", "a", "b", "c"]


@pytest.mark.parametrize("fold", FOLDS)
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_cases(case, fold, sim_library, both_beam_kernels):  # noqa: F811
    from pyctcdecode_amd import ConfidenceOutputBeam, build_ctcdecoder

    dec = build_ctcdecoder(case["labels"], lm_path(case["lm"]), case["unigrams"], **case["build"])
    x = INPUTS[case["input"]]
    tokens = dec.decode_beams(x, token_frames=True, **case["decode"])
    out = dec.decode_beams(x, confidence=fold, **case["decode"])
    assert all(type(b) is ConfidenceOutputBeam for b in out)
    same_but_for_confidence(out, tokens)
    n = check_logp(out, dec._alphabet.labels, log_probs(x), fold, TOL_F64, case["name"])
    assert n == sum(len(b.token_frames) for b in tokens)
    assert n > 0 or not any(b.text for b in out)


@pytest.mark.parametrize("fold", FOLDS)
def test_multi_lm_golden_cases(fold, sim_library):  # noqa: F811
    from tests.test_multi_lm import CASES as MULTI, INPUTS as MULTI_IN, build_product_multi

    for case in MULTI:
        dec, _ = build_product_multi(case)
        x = MULTI_IN[case["input"]]
        out = dec.decode_beams(x, confidence=fold, **case["decode"])
        same_but_for_confidence(out, dec.decode_beams(x, token_frames=True, **case["decode"]))
        check_logp(out, dec._alphabet.labels, log_probs(x), fold, TOL_F64, case["name"])


@pytest.mark.parametrize("fold", FOLDS)
@pytest.mark.parametrize("case", PROB_CASES, ids=lambda c: c["name"])
def test_probability_input(case, fold, sim_library):  # noqa: F811
    from pyctcdecode_amd import build_ctcdecoder

    labels = list(synth.LIBRI_LABELS if case["labels"] == "libri" else PROB_LABELS)
    dec = build_ctcdecoder(labels, TOY_ARPA if case["lm"] else None)
    x = PROB_INPUTS[case["name"]]
    out = dec.decode_beams(x, confidence=fold, **case["decode"])
    same_but_for_confidence(out, dec.decode_beams(x, token_frames=True, **case["decode"]))
    # (float32 / float16 inputs: the probability test in their own dtype, their tolerance class)
    assert x.dtype != np.float64
    check_logp(out, dec._alphabet.labels, lp_matrix(x), fold, tol_of(x.dtype), case["name"])


def _known_input():
    """'a' held for three frames with another probability each frame, a blank, 'a' again, 'b', a space, and the two-token
    word 'cb'. Whatever a frame's label leaves goes to the blank, which a token prune at KNOWN_MIN_LOGP (p >= 0.497) drops
    from every such frame: the beam has one way through them, as on a one-hot input, but its labels' values differ."""
    seq = [("a", 0.9), ("a", 0.6), ("a", 0.8), (None, 1.0), ("a", 0.7), ("b", 0.55), (" ", 0.9), ("c", 0.65), ("b", 0.85)]
    p = np.full((len(seq), len(CHARS)), 1e-9)
    for t, (lab, q) in enumerate(seq):
        if lab is not None:
            p[t, CHARS.index(lab)] = q
        p[t, 0] = 1.0 - p[t, 1:].sum()
    return np.log(p)


KNOWN_MIN_LOGP = -0.7


def test_known_folds(sim_library, both_beam_kernels):  # noqa: F811
    from pyctcdecode_amd import build_ctcdecoder

    dec = build_ctcdecoder(CHARS)
    x = _known_input()
    lp = log_probs(x)
    a, b, c = CHARS.index("a"), CHARS.index("b"), CHARS.index("c")
    runs = [lp[0:3, a], lp[4:5, a], lp[5:6, b], lp[7:8, c], lp[8:9, b]]
    want = {"mean": [float(np.sum(r)) / len(r) for r in runs], "min": [float(r.min()) for r in runs],
            "max": [float(r.max()) for r in runs]}
    # the folds differ where a token spans several frames, and only there
    held = [want[f][0] for f in FOLDS]
    assert len(set(held)) == 3 and want["min"][0] < want["mean"][0] < want["max"][0]
    assert want["mean"][0] == pytest.approx(math.log(0.9 * 0.6 * 0.8) / 3, abs=1e-8)
    for fold in FOLDS:
        best = dec.decode_beams(x, token_min_logp=KNOWN_MIN_LOGP, confidence=fold)[0]
        assert best.text == "aab cb"
        assert best.token_frames == [("a", (0, 3)), ("a", (4, 5)), ("b", (5, 6)), ("c", (7, 8)), ("b", (8, 9))]
        assert best.text_frames == [("aab", (0, 6)), ("cb", (7, 9))]
        assert best.token_logp == pytest.approx(want[fold], abs=TOL_F64)
        # a word is as sure as its least sure token: 'b' (0.55) of 'aab', 'c' (0.65) of the two-token word 'cb'
        assert best.word_logp == [min(best.token_logp[:3]), min(best.token_logp[3:])]
        assert best.word_logp[1] == best.token_logp[3] < best.token_logp[4]
        assert best.word_logp[0] == best.token_logp[2]
        check_logp([best], CHARS, lp, fold, TOL_F64)
        texts, tf = dec.decode_batch(None, [x], token_min_logp=KNOWN_MIN_LOGP, confidence=fold)
        assert texts == ["aab cb"] and tf.of(0) == best.token_frames and tf.logp_of(0) == best.token_logp


def _batch(n=9):
    lens = [61, 7, 33, 90, 2, 90, 45, 12, 70][:n]
    return [synth.d_words(2, u, t, synth.LIBRI_LABELS, False, LM.words, LM.sentences, 28, boost=4.0) for u, t in enumerate(lens)]


@pytest.mark.parametrize("fold", FOLDS)
def test_decode_batch_arrays_are_the_best_beams(fold, sim_library, both_beam_kernels):  # noqa: F811
    from pyctcdecode_amd import TokenFrames, build_ctcdecoder

    dec = build_ctcdecoder(synth.LIBRI_LABELS, LM.path)
    xs = _batch()
    hot = LM.hotwords(4, 1)  # (per-utterance lists need the HIP build: tests/test_gpu_token_logp.py)
    texts, tf = dec.decode_batch(None, xs, beam_width=24, hotwords=hot, confidence=fold)
    assert isinstance(tf, TokenFrames) and len(tf) == len(xs)
    assert tf.logp.dtype == np.float64 and tf.logp.shape == tf.label.shape and tf.offsets[-1] == len(tf.logp)
    assert texts == dec.decode_batch(None, xs, beam_width=24, hotwords=hot)
    t1, tf1 = dec.decode_batch(None, xs, beam_width=24, hotwords=hot, token_frames=True)
    assert t1 == texts and tf1.logp is None
    assert all(np.array_equal(getattr(tf, k), getattr(tf1, k)) for k in ("label", "start", "end", "offsets"))
    beams = dec.decode_beams_batch(None, xs, beam_width=24, hotwords=hot, prune_history=True, confidence=fold)
    same = dec.decode_beams_batch(None, xs, beam_width=24, hotwords=hot, prune_history=True, token_frames=True)
    for i, bs in enumerate(beams):
        same_but_for_confidence(bs, same[i])
        assert tf.of(i) == bs[0].token_frames and tf.logp_of(i) == bs[0].token_logp and texts[i] == bs[0].text
        check_logp(bs, dec._alphabet.labels, lp_matrix(xs[i]), fold, tol_of(xs[i].dtype), "utt %d" % i)  # (float32 rows)
    # a padded [B, T, V] batch (the zero rows of the padding are decoded as frames too)
    T = max(len(x) for x in xs)
    pad = np.zeros((len(xs), T, xs[0].shape[1]))  # (float64)
    for i, x in enumerate(xs):
        pad[i, : len(x)] = x
    t2, tf2 = dec.decode_batch(None, pad, beam_width=24, confidence=fold)
    assert t2 == dec.decode_batch(None, pad, beam_width=24)
    b2 = dec.decode_beams_batch(None, list(pad), beam_width=24, prune_history=True, confidence=fold)
    for i in range(len(xs)):
        assert tf2.of(i) == b2[i][0].token_frames and tf2.logp_of(i) == b2[i][0].token_logp
        check_token_logp(tf2.of(i), tf2.logp_of(i), dec._alphabet.labels, log_probs(pad[i]), fold, TOL_F64, "padded %d" % i)
    # the arrays pickle and join with their confidences
    back = pickle.loads(pickle.dumps(tf))
    assert np.array_equal(back.logp, tf.logp) and back.of(3) == tf.of(3)
    joined = TokenFrames.join([tf, tf2], dec._alphabet.labels)
    assert np.array_equal(joined.logp, np.concatenate([tf.logp, tf2.logp])) and joined.logp_of(len(xs) + 1) == tf2.logp_of(1)
    assert TokenFrames.join([tf, tf1], dec._alphabet.labels).logp is None


def test_sliced_host_ingest_gives_the_same_confidences(sim_library, monkeypatch):  # noqa: F811
    from pyctcdecode_amd import build_ctcdecoder

    dec = build_ctcdecoder(synth.LIBRI_LABELS, LM.path)
    xs = [x.astype(np.float32) for x in _batch()]
    hot = LM.hotwords(4, 1)
    kw = dict(beam_width=24, hotwords=hot, confidence="mean")
    monkeypatch.setenv("CTCDEC_HOST_SLICES", "0")
    whole = dec.decode_beams_batch(None, xs, prune_history=True, **kw)
    tw, fw = dec.decode_batch(None, xs, **kw)
    for i, bs in enumerate(whole):
        check_logp(bs, dec._alphabet.labels, lp_matrix(xs[i]), "mean", TOL_LOW, "utt %d" % i)
    for slices in (2, 3, 7):
        monkeypatch.setenv("CTCDEC_HOST_SLICES", str(slices))
        sliced = dec.decode_beams_batch(None, xs, prune_history=True, **kw)
        assert [[(b.text, b.token_frames, b.token_logp, b.word_logp) for b in bs] for bs in whole] == \
            [[(b.text, b.token_frames, b.token_logp, b.word_logp) for b in bs] for bs in sliced], slices
        ts, fs = dec.decode_batch(None, xs, **kw)
        assert ts == tw
        assert all(np.array_equal(getattr(fs, k), getattr(fw, k)) for k in ("label", "start", "end", "offsets", "logp"))


def test_device_pool_rebases_offsets(sim_library):  # noqa: F811
    from pyctcdecode_amd import ConfidenceOutputBeam, build_ctcdecoder
    from pyctcdecode_amd.parallel import DevicePool

    dec = build_ctcdecoder(synth.LIBRI_LABELS)
    xs = _batch()
    texts, tf = dec.decode_batch(None, xs, beam_width=16, confidence="min")
    beams = dec.decode_beams_batch(None, xs, beam_width=16, confidence="min")
    with DevicePool(dec, devices=[0, 0, 0], library=sim_library.path) as pool:
        pt, pf = dec.decode_batch(pool, xs, beam_width=16, confidence="min")
        pb = dec.decode_beams_batch(pool, xs, beam_width=16, confidence="min")
    assert pt == texts
    for k in ("label", "start", "end", "offsets", "logp"):
        assert np.array_equal(getattr(pf, k), getattr(tf, k)), k
    assert pf.logp.dtype == np.float64
    assert all(type(b) is ConfidenceOutputBeam for bs in pb for b in bs)
    key = lambda b: (b.text, b.token_frames, b.token_logp, b.word_logp)  # noqa: E731
    assert [[key(b) for b in bs] for bs in pb] == [[key(b) for b in bs] for bs in beams]
    for i, bs in enumerate(pb):
        check_logp(bs, dec._alphabet.labels, lp_matrix(xs[i]), "min", tol_of(xs[i].dtype), "utt %d" % i)


def test_defaults_are_unchanged(sim_library):  # noqa: F811
    from pyctcdecode_amd import ConfidenceOutputBeam, TokenFrames, TokenOutputBeam, build_ctcdecoder
    from pyctcdecode_amd.decoder import OutputBeam

    dec = build_ctcdecoder(synth.LIBRI_LABELS, LM.path)
    xs = _batch(3)
    for flag in ({}, {"confidence": None}):
        assert all(type(b) is OutputBeam for b in dec.decode_beams(xs[0], **flag))
        assert all(type(b) is OutputBeam for bs in dec.decode_beams_batch(None, xs, **flag) for b in bs)
        texts = dec.decode_batch(None, xs, **flag)
        assert isinstance(texts, list) and all(isinstance(t, str) for t in texts)
        assert all(type(b) is TokenOutputBeam for b in dec.decode_beams(xs[0], token_frames=True, **flag))
        _t, tf = dec.decode_batch(None, xs, token_frames=True, **flag)
        assert type(tf) is TokenFrames and tf.logp is None
        with pytest.raises(ValueError):
            tf.logp_of(0)
    cb = dec.decode_beams(xs[0], confidence="max")[0]
    assert isinstance(cb, ConfidenceOutputBeam) and isinstance(cb, TokenOutputBeam)
    safe = cb.get_mp_safe_beam()
    assert type(safe) is ConfidenceOutputBeam and safe.token_logp == cb.token_logp and safe.word_logp == cb.word_logp
    assert all(isinstance(v, float) for v in cb.token_logp + cb.word_logp)
    texts, tf = dec.decode_batch(None, [], confidence="mean")
    assert texts == [] and tf.logp is not None and len(tf.logp) == 0


def test_unknown_fold_is_refused(sim_library):  # noqa: F811
    from pyctcdecode_amd import build_ctcdecoder

    dec = build_ctcdecoder(synth.LIBRI_LABELS)
    xs = _batch(2)
    for bad in ("median", "", True, 2):
        with pytest.raises(ValueError):
            dec.decode_beams(xs[0], confidence=bad)
        with pytest.raises(ValueError):
            dec.decode_beams_batch(None, xs, confidence=bad)
        with pytest.raises(ValueError):
            dec.decode_batch(None, xs, confidence=bad)


def test_sharded_helpers_refuse(sim_library):  # noqa: F811
    from pyctcdecode_amd import build_ctcdecoder
    from pyctcdecode_amd.parallel import decode_batch_sharded, decode_beams_batch_sharded

    dec = build_ctcdecoder(synth.LIBRI_LABELS)
    with pytest.raises(NotImplementedError):
        decode_batch_sharded(dec, _batch(2), confidence="mean")
    with pytest.raises(NotImplementedError):
        decode_beams_batch_sharded(dec, _batch(2), confidence="mean")


def test_result_without_a_fold_has_no_confidences(sim_library):  # noqa: F811
    from pyctcdecode_amd import _binding as B
    from pyctcdecode_amd import build_ctcdecoder

    dec = build_ctcdecoder(CHARS)
    x = _known_input()
    for flag in (0, 1):
        params = dec._params(8, -10.0, -5.0, False, 10.0, 0)
        params.token_frames = flag
        res = dec._run([x], params, None)
        try:
            with pytest.raises((ValueError, B.NativeError)):
                dec._token_logp(res)
        finally:
            dec._lib.dll.ctcdec_result_free(res)
    params = dec._params(8, -10.0, -5.0, False, 10.0, 0)
    params.token_frames = 2  # CTCDEC_TOKEN_LOGP_MEAN
    res = dec._run([x], params, None)
    try:
        tf = dec._token_frames(res, len(dec._unpack(res, False)[0]), True)
        assert len(tf.logp) == len(tf.label) > 0
    finally:
        dec._lib.dll.ctcdec_result_free(res)
