"""GPU: the wave kernel's hash match and merge-free passes (csrc/beam_wave.h) on inputs that merge in most frames -- the
inputs of tests/test_wave_match.py, three utterances each: the wave and the workgroup kernel agree beam for beam, and both
with the oracle (strict order, scores within 1e-9); and a 64-utterance slice of the bench generator, text for text between
the two kernels."""
import os

import numpy as np
import pytest

from tests import wave_match_util as U

pytestmark = pytest.mark.gpu


def _decode(dec, kernel, code, xs, kw, monkeypatch):
    monkeypatch.setenv("CTCDEC_BEAM_KERNEL", kernel)
    out = dec.decode_beams_batch(None, [np.array(x) for x in xs], **kw)
    assert dec.last_beam_kernel == code
    return [U.beams_of(o) for o in out]


@pytest.mark.parametrize("name", sorted(U.CASES))
def test_wave_and_group_kernels_agree_on_merging_inputs(name, monkeypatch):
    from pyctcdecode_amd import build_ctcdecoder

    labels, _, kw = U.CASES[name]
    dec = build_ctcdecoder(labels)
    wave = _decode(dec, "wave", 1, U.inputs(name), kw, monkeypatch)
    group = _decode(dec, "group", 2, U.inputs(name), kw, monkeypatch)
    for u, want in enumerate(U.expected(name)):
        U.assert_same_beams(wave[u], group[u], "%s[%d] wave against group" % (name, u))
        U.assert_same_beams(wave[u], want, "%s[%d] wave" % (name, u))
        U.assert_same_beams(group[u], want, "%s[%d] group" % (name, u))


def test_bench_slice_texts_agree_between_the_kernels(tmp_path, monkeypatch):
    import bench
    from pyctcdecode_amd import build_ctcdecoder

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cache = os.path.join(root, "bench_cache") if os.access(root, os.W_OK) else str(tmp_path)
    lm, labels, hot = bench.build_assets(cache, 20000, 60000)
    xs = bench.make_batch(lm, labels, 0, 64, 60, 6.0, 1)
    dec = build_ctcdecoder(labels, lm.path)
    texts = {}
    for kernel, code in (("wave", 1), ("group", 2)):
        monkeypatch.setenv("CTCDEC_BEAM_KERNEL", kernel)
        texts[kernel] = dec.decode_batch(None, xs, beam_width=bench.BEAM, hotwords=hot)
        assert dec.last_beam_kernel == code
    assert len(texts["wave"]) == 64 and any(texts["wave"])
    for u, (a, b) in enumerate(zip(texts["wave"], texts["group"])):
        assert a == b, "utterance %d: wave %r, group %r" % (u, a, b)
