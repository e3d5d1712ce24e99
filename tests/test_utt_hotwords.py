"""Per-utterance hot words (decode_batch / decode_beams_batch with one hot-word list per utterance, ctcdec_set_hotword_sets):
the accepted and refused argument forms, the deduplication into sets, the slicing of the sharded helpers and of DevicePool, the
new symbol in both builds, and the simulator backend's refusal (its kernels run with the call-wide set only). The decodes
themselves are checked on the GPU: tests/test_gpu_utt_hotwords.py."""
import os

import numpy as np
import pytest

import synth
from tests.golden_util import LM_DIR
from tests.sim_util import sim_library  # noqa: F401


def test_argument_forms():
    from pyctcdecode_amd.decoder import _per_utt_hot

    assert _per_utt_hot(None, 10.0, 3) is None
    assert _per_utt_hot(["alpha", "beta gamma"], 10.0, 3) is None  # one shared list
    assert _per_utt_hot((w for w in ["alpha", "beta"]), 10.0, 3) is None  # a generator of str: still one shared list
    assert _per_utt_hot([], 10.0, 3) is None
    with pytest.raises(TypeError):
        _per_utt_hot(["alpha", ["beta"], None], 10.0, 3)  # str mixed with lists
    with pytest.raises(TypeError):
        _per_utt_hot([["alpha"], 5, None], 10.0, 3)  # an entry that is not a list of str
    with pytest.raises(ValueError):
        _per_utt_hot([["alpha"], None], 10.0, 3)  # wrong length
    with pytest.raises(ValueError):
        _per_utt_hot(["alpha"], [1.0, 2.0], 3)  # wrong number of weights
    sets, utt = _per_utt_hot([[" alpha ", "", "beta gamma"], None, ("delta",)], 10.0, 3)
    assert sets == [(("alpha", "beta", "gamma"), 10.0), (("delta",), 10.0)]  # normalised like HotwordScorer.build_scorer
    assert utt == [0, -1, 1]
    # per-utterance weights with a shared list
    sets, utt = _per_utt_hot(["alpha"], np.array([1.0, 0.0, 1.0]), 3)
    assert sets == [(("alpha",), 1.0), (("alpha",), 0.0)] and utt == [0, 1, 0]


def test_deduplication():
    from pyctcdecode_amd.decoder import BeamSearchDecoderCTC, _per_utt_hot

    sets, utt = _per_utt_hot([["a", "b"], ["c"], ["a", "b"], ["a  b"], ["c"]], [1.0, 2.0, 1.0, 1.0, 3.0], 5)
    assert sets == [(("a", "b"), 1.0), (("c",), 2.0), (("c",), 3.0)]
    assert utt == [0, 1, 0, 0, 2]
    # one list for every utterance: one set, and the batch goes the call-wide way
    resolve = BeamSearchDecoderCTC._resolve_hot
    assert resolve(None, [["x", "y"]] * 4, 7.0, 4) == (["x", "y"], 7.0, None)
    assert resolve(None, [["x"]] * 2, [2.0, 2.0], 2) == (["x"], 2.0, None)
    assert resolve(None, [None, []], 7.0, 2)[2] is None
    assert resolve(None, ["x"], 7.0, 2) == (["x"], 7.0, None)
    hw, w, hot = resolve(None, [["x"], None], 7.0, 2)
    assert hot == ([(("x",), 7.0)], [0, -1])


def test_shard_slicing():
    from pyctcdecode_amd.parallel import _hot_kwargs, _slice_kwargs

    kw = _hot_kwargs({"hotwords": [["a"], None, ["b"], ["c"]], "hotword_weight": np.array([1.0, 2.0, 3.0, 4.0]), "beam_width": 8}, 4)
    part = _slice_kwargs(kw, 1, 3)
    assert part == {"hotwords": [None, ["b"]], "hotword_weight": [2.0, 3.0], "beam_width": 8}
    shared = _hot_kwargs({"hotwords": (w for w in ["a", "b"]), "hotword_weight": 5.0}, 4)
    assert shared["hotwords"] == ["a", "b"]
    assert _slice_kwargs(shared, 1, 3) == {"hotwords": ["a", "b"], "hotword_weight": 5.0}
    with pytest.raises(ValueError):
        _hot_kwargs({"hotwords": [["a"], None]}, 4)
    with pytest.raises(TypeError):
        _hot_kwargs({"hotwords": ["a", ["b"]]}, 2)


class _Conn:
    """Stands in for a DevicePool worker's pipe: records what it is sent and answers with the hot words it got."""

    def __init__(self):
        self.sent = []

    def send(self, msg):
        self.sent.append(msg)

    def recv(self):
        method, xs, kw = self.sent[-1]
        hw, w = kw.get("hotwords"), kw.get("hotword_weight")
        return "ok", [(len(x), hw[i] if isinstance(hw, list) and hw and not isinstance(hw[0], str) else hw,
                       w[i] if isinstance(w, list) else w) for i, x in enumerate(xs)]


def test_device_pool_slices_hot_words():
    from pyctcdecode_amd.parallel import DevicePool

    pool = DevicePool.__new__(DevicePool)
    conns = [_Conn(), _Conn()]
    pool._workers = [(None, c) for c in conns]
    xs = [np.zeros((t, 3), np.float32) for t in (10, 10, 10, 10)]
    hot = [["a"], None, ["b"], ["c", "d"]]
    got = pool._map("decode_batch", xs, {"hotwords": hot, "hotword_weight": [1.0, 2.0, 3.0, 4.0]})
    assert got == [(10, ["a"], 1.0), (10, None, 2.0), (10, ["b"], 3.0), (10, ["c", "d"], 4.0)]
    assert [len(c.sent[0][1]) for c in conns] == [2, 2]
    # a generator of hot words is materialised before it is pickled
    got = pool._map("decode_batch", xs, {"hotwords": (w for w in ["x", "y"]), "hotword_weight": 5.0})
    assert [g[1] for g in got] == [["x", "y"]] * 4
    import pickle

    pickle.dumps(conns[0].sent[-1])
    pool._workers = []


def test_symbol_in_both_builds():
    from pyctcdecode_amd import _binding as B
    from pyctcdecode_amd import build as _build
    from tests.sim.build_sim import build as build_sim

    for path in (_build.build(), build_sim()):
        lib = B.Library(path)
        assert hasattr(lib.dll, "ctcdec_set_hotword_sets"), path


def test_simulator_refuses_per_utterance_sets(sim_library):  # noqa: F811
    from pyctcdecode_amd import build_ctcdecoder

    lm = synth.SynthLM(LM_DIR, 300, 400, order=4, seed=2)
    dec = build_ctcdecoder(synth.LIBRI_LABELS, lm.path)
    xs = [synth.d_words(2, u, t, synth.LIBRI_LABELS, False, lm.words, lm.sentences, 28, boost=4.0) for u, t in enumerate([20, 12])]
    hot = lm.hotwords(3, 1)
    with pytest.raises(NotImplementedError, match="per-utterance hot words"):
        dec.decode_beams_batch(None, xs, beam_width=8, hotwords=[hot, None])
    with pytest.raises(NotImplementedError):
        dec.decode_batch(None, xs, beam_width=8, hotwords=hot, hotword_weight=[1.0, 2.0])
    # nothing is left armed: the next calls are the shared-list calls they always were, and the same list given per
    # utterance is one set on the call-wide path
    shared = dec.decode_beams_batch(None, xs, beam_width=8, hotwords=hot)
    per = dec.decode_beams_batch(None, xs, beam_width=8, hotwords=[hot, list(hot)])
    key = lambda bs: [[(b.text, b.text_frames, b.logit_score, b.lm_score) for b in x] for x in bs]  # noqa: E731
    assert key(per) == key(shared)
    assert key(shared) == [key([dec.decode_beams(x, beam_width=8, hotwords=hot)])[0] for x in xs]
