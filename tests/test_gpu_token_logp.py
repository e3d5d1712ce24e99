"""GPU (-m gpu): token and word confidences (confidence=...) on the HIP build, whose token_logp kernel reads the survivor lists
the frame-prune stage of the same call left on the device. Every token of every beam of the committed reference goldens under
both beam kernels against the numpy fold of the frame prune's own matrix; device tensors of every dtype; a launch of more than
2048 utterances whose confidences agree between the wave kernel, the workgroup kernel and the CPU simulator; a 4096-utterance
decode_batch(confidence="mean"). No token is left out of a check."""
import numpy as np
import pytest
import torch

import synth
from tests.golden_util import LM_DIR, lm_path, load_cases
from tests.token_frames_util import log_probs
from tests.token_logp_util import FOLDS, TOL_F64, TOL_LOW, check_logp, check_token_logp, lp_matrix, same_but_for_confidence

pytestmark = pytest.mark.gpu

CASES, INPUTS = load_cases()
LABELS = synth.LIBRI_LABELS


@pytest.fixture(scope="module")
def lm():
    return synth.SynthLM(LM_DIR, 300, 400, order=4, seed=2)


def _inputs(lm, n, seed=0, lo=20, hi=120):
    rng = np.random.default_rng(seed)
    out = []
    for u, t in enumerate(rng.integers(lo, hi, size=n)):
        out.append(synth.d_words(2, u + 7 * seed, int(t), LABELS, False, lm.words, lm.sentences, 28, boost=4.0))
    return out


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_cases(case, both_beam_kernels):
    from pyctcdecode_amd import ConfidenceOutputBeam, build_ctcdecoder

    dec = build_ctcdecoder(case["labels"], lm_path(case["lm"]), case["unigrams"], **case["build"])
    x = INPUTS[case["input"]]
    assert x.dtype not in (np.float32, np.float16)  # (float64, or integers that go to the device as float64: its tolerance)
    lp = log_probs(x)
    tokens = dec.decode_beams(x, token_frames=True, **case["decode"])
    for fold in FOLDS:
        out = dec.decode_beams(x, confidence=fold, **case["decode"])
        assert all(type(b) is ConfidenceOutputBeam for b in out)
        same_but_for_confidence(out, tokens)
        n = check_logp(out, dec._alphabet.labels, lp, fold, TOL_F64, "%s %s" % (case["name"], fold))
        assert n == sum(len(b.token_frames) for b in tokens)


@pytest.mark.parametrize("fold", FOLDS)
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32, torch.float64])
def test_device_tensors(lm, dtype, fold):
    from pyctcdecode_amd import build_ctcdecoder

    dec = build_ctcdecoder(LABELS, lm.path)
    xs = _inputs(lm, 12, seed=3)
    dev = [torch.from_numpy(x).to(dtype).cuda() for x in xs]
    tol = TOL_F64 if dtype == torch.float64 else TOL_LOW
    hot = [lm.hotwords(4, 1) if i % 2 else lm.hotwords(3, 2, seed=5) for i in range(len(dev))]  # (one list per utterance)
    for hotwords in (lm.hotwords(4, 1), hot):
        beams = dec.decode_beams_batch(None, dev, beam_width=32, hotwords=hotwords, confidence=fold)
        same = dec.decode_beams_batch(None, dev, beam_width=32, hotwords=hotwords, token_frames=True)
        texts, tf = dec.decode_batch(None, dev, beam_width=32, hotwords=hotwords, confidence=fold)
        assert texts == dec.decode_batch(None, dev, beam_width=32, hotwords=hotwords)
        assert tf.logp.dtype == np.float64 and len(tf.logp) == len(tf.label) == tf.offsets[-1]
        for i, bs in enumerate(beams):
            lp = log_probs(dev[i].double().cpu().numpy())
            same_but_for_confidence(bs, same[i])
            check_logp(bs, dec._alphabet.labels, lp, fold, tol, "%s utt %d" % (dtype, i))
            check_token_logp(tf.of(i), tf.logp_of(i), dec._alphabet.labels, lp, fold, tol, "%s decode_batch utt %d" % (dtype, i))
    one = dec.decode_beams(dev[0], confidence=fold)
    same_but_for_confidence(one, dec.decode_beams(dev[0], token_frames=True))
    check_logp(one, dec._alphabet.labels, log_probs(dev[0].double().cpu().numpy()), fold, tol)


def test_full_launch_both_kernels_and_simulator(lm, monkeypatch):
    from pyctcdecode_amd import _binding as B
    from pyctcdecode_amd import build_ctcdecoder
    from tests.sim.build_sim import build

    dec = build_ctcdecoder(LABELS, lm.path)
    fillers = _inputs(lm, 536, seed=5)
    golden = [c for c in CASES if c["labels"] == list(LABELS) and not c["decode"].get("hotwords")]
    xs = [fillers[u % len(fillers)] for u in range(2048 + 96)]
    places = {0: 0, len(xs) - 1: 1, 1024: 2, 2047: 3}
    for p, g in places.items():
        if g < len(golden):
            xs[p] = INPUTS[golden[g]["input"]]
    kw = dict(beam_width=64, hotwords=lm.hotwords(4, 1), prune_history=True, confidence="mean")
    got, logp = {}, {}
    for kernel in ("wave", "group"):
        monkeypatch.setenv("CTCDEC_BEAM_KERNEL", kernel)
        out = dec.decode_beams_batch(None, xs, **kw)
        got[kernel] = [[(b.text, b.token_frames) for b in bs] for bs in out]
        logp[kernel] = [[(b.token_logp, b.word_logp) for b in bs] for bs in out]
        if kernel == "wave":
            assert dec.last_beam_kernel == 1
            for i in list(places) + list(range(3, len(xs), 97)):
                x = np.asarray(xs[i])
                check_logp(out[i], dec._alphabet.labels, lp_matrix(x), "mean", TOL_F64 if x.dtype == np.float64 else TOL_LOW,
                           "utt %d" % i)
    assert got["wave"] == got["group"]

    def close(a, b):
        assert len(a) == len(b)
        for ba, bb in zip(a, b):
            assert len(ba) == len(bb)
            for (ta, wa), (tb, wb) in zip(ba, bb):
                assert len(ta) == len(tb) and len(wa) == len(wb)
                assert all(abs(p - q) <= 1e-9 for p, q in zip(ta, tb)) and all(abs(p - q) <= 1e-9 for p, q in zip(wa, wb))

    close(logp["wave"], logp["group"])
    # the same utterances on the CPU simulator of the kernels (decoded there in a batch of their own)
    sample = sorted(set(list(places) + list(range(5, len(xs), 211))))
    monkeypatch.delenv("CTCDEC_BEAM_KERNEL")
    monkeypatch.setattr(B, "_LIB", B.Library(build()))
    sim = build_ctcdecoder(LABELS, lm.path)
    out = sim.decode_beams_batch(None, [xs[i] for i in sample], **kw)
    assert [[(b.text, b.token_frames) for b in bs] for bs in out] == [got["wave"][i] for i in sample]
    close([[(b.token_logp, b.word_logp) for b in bs] for bs in out], [logp["wave"][i] for i in sample])


def test_decode_batch_4096(lm):
    from pyctcdecode_amd import build_ctcdecoder

    dec = build_ctcdecoder(LABELS, lm.path)
    base = _inputs(lm, 256, seed=9, lo=60, hi=200)
    xs = [torch.from_numpy(base[u % len(base)]).float().cuda() for u in range(4096)]
    kw = dict(beam_width=32, hotwords=lm.hotwords(4, 1))
    plain = dec.decode_batch(None, xs, **kw)
    texts, tf = dec.decode_batch(None, xs, confidence="mean", **kw)
    assert texts == plain
    assert len(tf) == 4096 and tf.offsets[-1] == len(tf.label) == len(tf.logp) and tf.logp.dtype == np.float64
    sample = list(range(0, 4096, 509))
    beams = dec.decode_beams_batch(None, [xs[i] for i in sample], prune_history=True, confidence="mean", **kw)
    for i, bs in zip(sample, beams):
        assert tf.of(i) == bs[0].token_frames and tf.logp_of(i) == bs[0].token_logp and texts[i] == bs[0].text, i
        check_logp(bs, dec._alphabet.labels, log_probs(xs[i].double().cpu().numpy()), "mean", TOL_LOW, "utt %d" % i)
