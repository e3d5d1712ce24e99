"""Per-token frames of the returned beams (token_frames=True on decode_beams / decode_beams_batch / decode_batch) on the CPU
simulator of the beam kernels: the contract of DESIGN.md "Token frames" on every beam of the committed reference goldens (their
word frames are the reference's, so property 1 ties the tokens to it), exact token lists on hand-built one-hot inputs, the
array form of decode_batch, time-sliced host ingest, DevicePool and the unchanged defaults. The HIP build:
tests/test_gpu_token_frames.py."""
import json
import os

import numpy as np
import pytest

import synth
from tests.golden_util import GOLD, LM_DIR, TOY_ARPA, lm_path, load_cases
from tests.sim_util import sim_library  # noqa: F401
from tests.token_frames_util import check_beams, log_probs

CASES, INPUTS = load_cases()
with open(os.path.join(GOLD, "cases_probs.json")) as _f:
    PROB_CASES = json.load(_f)["cases"]
PROB_INPUTS = np.load(os.path.join(GOLD, "inputs_probs.npz"))
PROB_LABELS = [" ", "b", "g", "n", "s", "u", "y", ""]
LM = synth.SynthLM(LM_DIR, 300, 400, order=4, seed=2)

CHARS = ["", " ", "a", "b", "c"]
BPE = ["", "▁a", "b", "▁", "▁⁇▁", "▁c"]


def _one_hot(labels, seq):
    """log-probabilities with one label per frame (None: blank) and nothing else within reach of the token prune"""
    x = np.full((len(seq), len(labels)), -30.0)
    for t, lab in enumerate(seq):
        x[t, labels.index("" if lab is None else lab)] = 0.0
    return x


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_cases_keep_the_contract(case, sim_library, both_beam_kernels):  # noqa: F811
    from pyctcdecode_amd import TokenOutputBeam, build_ctcdecoder

    dec = build_ctcdecoder(case["labels"], lm_path(case["lm"]), case["unigrams"], **case["build"])
    x = INPUTS[case["input"]]
    plain = dec.decode_beams(x, **case["decode"])
    out = dec.decode_beams(x, token_frames=True, **case["decode"])
    assert all(type(b) is TokenOutputBeam for b in out)
    assert [(b.text, list(b.text_frames), b.logit_score, b.lm_score) for b in out] == \
        [(b.text, list(b.text_frames), b.logit_score, b.lm_score) for b in plain]
    al = dec._alphabet
    check_beams(out, al.labels, al.is_bpe, log_probs(x), case["decode"].get("token_min_logp", -5.0), case["name"])
    assert any(b.token_frames for b in out) or not any(b.text for b in out)


def test_multi_lm_golden_cases(sim_library):  # noqa: F811
    from tests.test_multi_lm import CASES as MULTI, INPUTS as MULTI_IN, build_product_multi

    for case in MULTI:
        dec, _ = build_product_multi(case)
        x = MULTI_IN[case["input"]]
        out = dec.decode_beams(x, token_frames=True, **case["decode"])
        assert len(out) == len(case["expected"])
        check_beams(out, dec._alphabet.labels, dec._alphabet.is_bpe, log_probs(x), case["decode"].get("token_min_logp", -5.0),
                    case["name"])


@pytest.mark.parametrize("case", PROB_CASES, ids=lambda c: c["name"])
def test_probability_input(case, sim_library):  # noqa: F811
    from pyctcdecode_amd import build_ctcdecoder

    labels = list(synth.LIBRI_LABELS if case["labels"] == "libri" else PROB_LABELS)
    dec = build_ctcdecoder(labels, TOY_ARPA if case["lm"] else None)
    out = dec.decode_beams(PROB_INPUTS[case["name"]], token_frames=True, **case["decode"])
    check_beams(out, dec._alphabet.labels, dec._alphabet.is_bpe, None, what=case["name"])  # (properties 1 and 2)


CHAR_CASES = [
    # repeats, a blank-separated repeat, a double space
    (["a", "a", None, "a", "b", "b", " ", " ", "c", None], "aab c",
     [("a", (0, 2)), ("a", (3, 4)), ("b", (4, 6)), ("c", (8, 9))]),
    # leading and trailing spaces
    ([" ", "a", None, " ", "b", " "], "a b", [("a", (1, 2)), ("b", (4, 5))]),
    ([None, None, None], "", []),
]
BPE_CASES = [
    # a bare ▁ (empty word, forced break), ▁⁇▁ (forced break of the next label), a trailing bare ▁
    (["▁a", "b", "b", None, "▁", "▁", "▁c", "▁⁇▁", "b", None, "▁"], None,
     [("▁a", (0, 1)), ("b", (1, 3)), ("▁", (4, 6)), ("▁c", (6, 7)), ("▁⁇▁", (7, 8)), ("b", (8, 9)), ("▁", (10, 11))]),
    (["b", "▁a", None], None, [("b", (0, 1)), ("▁a", (1, 2))]),
    ([None], None, []),
]


@pytest.mark.parametrize("labels,cases", [(CHARS, CHAR_CASES), (BPE, BPE_CASES)], ids=["chars", "bpe"])
def test_known_token_lists(labels, cases, sim_library, both_beam_kernels):  # noqa: F811
    from pyctcdecode_amd import build_ctcdecoder

    dec = build_ctcdecoder(labels)
    for seq, text, want in cases:
        x = _one_hot(labels, seq)
        best = dec.decode_beams(x, token_frames=True)[0]
        if text is not None:
            assert best.text == text
        assert best.token_frames == want, (seq, best.token_frames)
        check_beams([best], dec._alphabet.labels, dec._alphabet.is_bpe, log_probs(x))
        texts, tf = dec.decode_batch(None, [x], token_frames=True)
        assert texts == [best.text] and tf.of(0) == want


def _batch(n=9):
    lens = [61, 7, 33, 90, 2, 90, 45, 12, 70][:n]
    return [synth.d_words(2, u, t, synth.LIBRI_LABELS, False, LM.words, LM.sentences, 28, boost=4.0) for u, t in enumerate(lens)]


def test_decode_batch_arrays_are_the_best_beams(sim_library, both_beam_kernels):  # noqa: F811
    from pyctcdecode_amd import TokenFrames, build_ctcdecoder

    dec = build_ctcdecoder(synth.LIBRI_LABELS, LM.path)
    xs = _batch()
    hot = LM.hotwords(4, 1)
    texts, tf = dec.decode_batch(None, xs, beam_width=24, hotwords=hot, token_frames=True)
    assert isinstance(tf, TokenFrames) and len(tf) == len(xs)
    assert tf.label.dtype == np.int32 and tf.start.dtype == np.int32 and tf.end.dtype == np.int32
    assert tf.offsets.dtype == np.int64 and tf.offsets.shape == (len(xs) + 1,) and tf.offsets[-1] == len(tf.label)
    assert texts == dec.decode_batch(None, xs, beam_width=24, hotwords=hot)
    beams = dec.decode_beams_batch(None, xs, beam_width=24, hotwords=hot, prune_history=True, token_frames=True)
    for i, bs in enumerate(beams):
        assert tf.of(i) == bs[0].token_frames and texts[i] == bs[0].text
        check_beams(bs, dec._alphabet.labels, False, log_probs(xs[i]), what="utt %d" % i)
    # a padded [B, T, V] batch
    T = max(len(x) for x in xs)
    pad = np.zeros((len(xs), T, xs[0].shape[1]))
    for i, x in enumerate(xs):
        pad[i, : len(x)] = x
    # (the zero rows of the padding are decoded as frames too: compare the arrays with the beams of the same input)
    t2, tf2 = dec.decode_batch(None, pad, beam_width=24, token_frames=True)
    assert t2 == dec.decode_batch(None, pad, beam_width=24)
    b2 = dec.decode_beams_batch(None, list(pad), beam_width=24, prune_history=True, token_frames=True)
    assert [tf2.of(i) for i in range(len(xs))] == [b[0].token_frames for b in b2]


def test_sliced_host_ingest_gives_the_same_tokens(sim_library, monkeypatch):  # noqa: F811
    from pyctcdecode_amd import build_ctcdecoder

    dec = build_ctcdecoder(synth.LIBRI_LABELS, LM.path)
    xs = [x.astype(np.float32) for x in _batch()]
    hot = LM.hotwords(4, 1)
    monkeypatch.setenv("CTCDEC_HOST_SLICES", "0")
    whole = dec.decode_beams_batch(None, xs, beam_width=24, hotwords=hot, prune_history=True, token_frames=True)
    tw, fw = dec.decode_batch(None, xs, beam_width=24, hotwords=hot, token_frames=True)
    for slices in (2, 3, 7):
        monkeypatch.setenv("CTCDEC_HOST_SLICES", str(slices))
        sliced = dec.decode_beams_batch(None, xs, beam_width=24, hotwords=hot, prune_history=True, token_frames=True)
        assert [[b.token_frames for b in bs] for bs in whole] == [[b.token_frames for b in bs] for bs in sliced], slices
        assert [[b.text for b in bs] for bs in whole] == [[b.text for b in bs] for bs in sliced], slices
        ts, fs = dec.decode_batch(None, xs, beam_width=24, hotwords=hot, token_frames=True)
        assert ts == tw and all(np.array_equal(getattr(fs, k), getattr(fw, k)) for k in ("label", "start", "end", "offsets"))


def test_defaults_are_unchanged(sim_library):  # noqa: F811
    from pyctcdecode_amd import TokenOutputBeam, build_ctcdecoder
    from pyctcdecode_amd.decoder import OutputBeam

    dec = build_ctcdecoder(synth.LIBRI_LABELS, LM.path)
    xs = _batch(3)
    for flag in ({}, {"token_frames": False}):
        assert all(type(b) is OutputBeam for b in dec.decode_beams(xs[0], **flag))
        assert all(type(b) is OutputBeam for bs in dec.decode_beams_batch(None, xs, **flag) for b in bs)
        texts = dec.decode_batch(None, xs, **flag)
        assert isinstance(texts, list) and all(isinstance(t, str) for t in texts)
    tb = dec.decode_beams(xs[0], token_frames=True)[0]
    assert isinstance(tb, TokenOutputBeam) and isinstance(tb, OutputBeam)
    assert tb.get_mp_safe_beam().token_frames == tb.token_frames
    assert dec.decode_batch(None, [], token_frames=True)[0] == []


def test_sharded_helpers_refuse(sim_library):  # noqa: F811
    from pyctcdecode_amd import build_ctcdecoder
    from pyctcdecode_amd.parallel import decode_batch_sharded, decode_beams_batch_sharded

    dec = build_ctcdecoder(synth.LIBRI_LABELS)
    with pytest.raises(NotImplementedError):
        decode_batch_sharded(dec, _batch(2), token_frames=True)
    with pytest.raises(NotImplementedError):
        decode_beams_batch_sharded(dec, _batch(2), token_frames=True)


def test_device_pool_rebases_offsets(sim_library):  # noqa: F811
    from pyctcdecode_amd import build_ctcdecoder
    from pyctcdecode_amd.parallel import DevicePool

    dec = build_ctcdecoder(synth.LIBRI_LABELS)
    xs = _batch()
    texts, tf = dec.decode_batch(None, xs, beam_width=16, token_frames=True)
    beams = dec.decode_beams_batch(None, xs, beam_width=16, token_frames=True)
    with DevicePool(dec, devices=[0, 0, 0], library=sim_library.path) as pool:
        pt, pf = dec.decode_batch(pool, xs, beam_width=16, token_frames=True)
        pb = dec.decode_beams_batch(pool, xs, beam_width=16, token_frames=True)
    assert pt == texts
    for k in ("label", "start", "end", "offsets"):
        assert np.array_equal(getattr(pf, k), getattr(tf, k)), k
    assert [[b.token_frames for b in bs] for bs in pb] == [[b.token_frames for b in bs] for bs in beams]


def test_result_without_the_flag_has_no_tokens(sim_library):  # noqa: F811
    from pyctcdecode_amd import build_ctcdecoder

    dec = build_ctcdecoder(CHARS)
    params = dec._params(8, -10.0, -5.0, False, 10.0, 0)
    res = dec._run([_one_hot(CHARS, ["a"])], params, None)
    try:
        with pytest.raises(ValueError):
            dec._token_frames(res, 1)
    finally:
        dec._lib.dll.ctcdec_result_free(res)
