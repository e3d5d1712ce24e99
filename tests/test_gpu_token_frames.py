"""GPU (-m gpu): per-token frames (token_frames=True) on the HIP build. The contract of DESIGN.md "Token frames" on every beam of
the committed reference goldens under both beam kernels and on float16 / bfloat16 device tensors; a launch of more than 2048
utterances whose token frames are the same under the wave and the workgroup kernel and equal the CPU simulator's; a
4096-utterance decode_batch(token_frames=True) whose texts equal the plain call's."""
import numpy as np
import pytest
import torch

import synth
from tests.golden_util import LM_DIR, lm_path, load_cases
from tests.token_frames_util import check_beams, log_probs

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
def test_golden_cases_keep_the_contract(case, both_beam_kernels):
    from pyctcdecode_amd import build_ctcdecoder

    dec = build_ctcdecoder(case["labels"], lm_path(case["lm"]), case["unigrams"], **case["build"])
    x = INPUTS[case["input"]]
    plain = dec.decode_beams(x, **case["decode"])
    out = dec.decode_beams(x, token_frames=True, **case["decode"])
    assert [(b.text, list(b.text_frames), b.logit_score, b.lm_score) for b in out] == \
        [(b.text, list(b.text_frames), b.logit_score, b.lm_score) for b in plain]
    al = dec._alphabet
    check_beams(out, al.labels, al.is_bpe, log_probs(x), case["decode"].get("token_min_logp", -5.0), case["name"])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float64])
def test_device_tensors(lm, dtype):
    from pyctcdecode_amd import build_ctcdecoder

    dec = build_ctcdecoder(LABELS, lm.path)
    xs = _inputs(lm, 12, seed=3)
    dev = [torch.from_numpy(x).to(dtype).cuda() for x in xs]
    beams = dec.decode_beams_batch(None, dev, beam_width=32, hotwords=lm.hotwords(4, 1), token_frames=True)
    texts, tf = dec.decode_batch(None, dev, beam_width=32, hotwords=lm.hotwords(4, 1), token_frames=True)
    assert texts == dec.decode_batch(None, dev, beam_width=32, hotwords=lm.hotwords(4, 1))
    for i, bs in enumerate(beams):
        x = dev[i].double().cpu().numpy()
        check_beams(bs, dec._alphabet.labels, False, log_probs(x), what="%s utt %d" % (dtype, i))
    one = dec.decode_beams(dev[0], token_frames=True)
    check_beams(one, dec._alphabet.labels, False, log_probs(dev[0].double().cpu().numpy()))


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
    kw = dict(beam_width=64, hotwords=lm.hotwords(4, 1), prune_history=True, token_frames=True)
    got = {}
    for kernel in ("wave", "group"):
        monkeypatch.setenv("CTCDEC_BEAM_KERNEL", kernel)
        out = dec.decode_beams_batch(None, xs, **kw)
        got[kernel] = [[(b.text, b.token_frames) for b in bs] for bs in out]
        if kernel == "wave":
            assert dec.last_beam_kernel == 1
            for i in list(places) + list(range(3, len(xs), 97)):
                check_beams(out[i], dec._alphabet.labels, False, log_probs(xs[i]), what="utt %d" % i)
    assert got["wave"] == got["group"]
    # the same utterances on the CPU simulator of the kernels (decoded there in a batch of their own)
    sample = sorted(set(list(places) + list(range(5, len(xs), 211))))
    monkeypatch.delenv("CTCDEC_BEAM_KERNEL")
    monkeypatch.setattr(B, "_LIB", B.Library(build()))
    sim = build_ctcdecoder(LABELS, lm.path)
    out = sim.decode_beams_batch(None, [xs[i] for i in sample], **kw)
    assert [[(b.text, b.token_frames) for b in bs] for bs in out] == [got["wave"][i] for i in sample]


def test_decode_batch_4096(lm):
    from pyctcdecode_amd import build_ctcdecoder

    dec = build_ctcdecoder(LABELS, lm.path)
    base = _inputs(lm, 256, seed=9, lo=60, hi=200)
    xs = [torch.from_numpy(base[u % len(base)]).float().cuda() for u in range(4096)]
    kw = dict(beam_width=32, hotwords=lm.hotwords(4, 1))
    plain = dec.decode_batch(None, xs, **kw)
    texts, tf = dec.decode_batch(None, xs, token_frames=True, **kw)
    assert texts == plain
    assert len(tf) == 4096 and tf.offsets[-1] == len(tf.label)
    sample = list(range(0, 4096, 509))
    beams = dec.decode_beams_batch(None, [xs[i] for i in sample], prune_history=True, token_frames=True, **kw)
    for i, bs in zip(sample, beams):
        assert tf.of(i) == bs[0].token_frames and texts[i] == bs[0].text, i
        check_beams(bs, dec._alphabet.labels, False, log_probs(xs[i].double().cpu().numpy()), what="utt %d" % i)
