"""GPU (-m gpu): per-utterance hot words on both beam kernels. Every utterance of a batch decoded with its own hot-word list
and weight equals the same utterance decoded alone with that list (texts, frames, scores, order -- bit for bit) and the
oracle; the same list given per utterance equals the shared list; the set follows the utterance through the placement of
large launches; per-stream scorers of partial_decode_beams_batch equal each stream run alone; DevicePool shards the lists."""
import numpy as np
import pytest
import torch

import synth
from oracle.ctc_oracle import build_oracle
from tests.golden_util import LM_DIR, check_beams

pytestmark = pytest.mark.gpu

LABELS = synth.LIBRI_LABELS


@pytest.fixture(scope="module")
def lm():
    return synth.SynthLM(LM_DIR, 300, 400, order=4, seed=2)


def _key(beams):
    return [(b.text, list(b.text_frames), b.logit_score, b.lm_score) for b in beams]


def _inputs(lm, n, seed=0):
    rng = np.random.default_rng(seed)
    ts = [0, 1] + [int(t) for t in rng.integers(8, 70, size=n - 2)]
    xs = []
    for u, t in enumerate(ts):
        x = synth.d_words(2, u + 11 * seed, max(t, 2), LABELS, False, lm.words, lm.sentences, 28, boost=4.0)
        xs.append(np.ascontiguousarray(x[:t]))
    return xs


def _hot_lists(lm, n):
    long_words = [w for w in lm.words if len(w) >= 5]
    w = long_words[0]
    shared = lm.hotwords(4, 1)
    kinds = [
        None,
        shared,
        ["zqxjv", "qqzzyy"],  # out of vocabulary
        [" ".join(lm.words[i] for i in lm.sentences[0][:2]), long_words[1]],  # a multi-word phrase
        [w[:3]],  # a prefix of the next set's word
        [w],
        [],
        lm.hotwords(6, 2, seed=5),
    ]
    weights = [10.0, 0.0, 3.5, 10.0, 7.0, 2.0, 10.0, 12.0]
    return [kinds[u % len(kinds)] for u in range(n)], [weights[(u // 2) % len(weights)] for u in range(n)]


def test_per_utterance_lists_match_single_calls_and_oracle(lm, both_beam_kernels):
    from pyctcdecode_amd import build_ctcdecoder
    from pyctcdecode_amd.alphabet import Alphabet

    dec = build_ctcdecoder(LABELS, lm.path)
    xs = _inputs(lm, 24)
    hot, wts = _hot_lists(lm, 24)
    got = dec.decode_beams_batch(None, xs, beam_width=16, hotwords=hot, hotword_weight=wts)
    alpha = Alphabet.build_alphabet(LABELS)
    orc = build_oracle(alpha.labels, alpha.is_bpe, lm.path, None)
    for u, x in enumerate(xs):
        alone = dec.decode_beams(x, beam_width=16, hotwords=hot[u], hotword_weight=wts[u])
        assert _key(got[u]) == _key(alone), u
        with np.errstate(all="ignore"):
            exp = orc.decode_beams(x, beam_width=16, hotwords=hot[u], hotword_weight=wts[u])
        exp = [{"text": o[0], "frames": [[w, int(a), int(b)] for w, (a, b) in o[2]], "logit": o[3], "lm": o[4]} for o in exp]
        check_beams([(o.text, o.text_frames, o.logit_score, o.lm_score) for o in got[u]], exp, what="utt%d" % u, tie_tol=0.0)
    texts = dec.decode_batch(None, xs, beam_width=16, hotwords=hot, hotword_weight=wts)
    assert texts == [g[0].text if g else "" for g in got]
    # the hot words changed the outcome somewhere (the test would show nothing otherwise)
    plain = dec.decode_beams_batch(None, xs, beam_width=16)
    assert any(_key(a) != _key(b) for a, b in zip(got, plain))


def test_shared_list_given_per_utterance_is_bit_identical(lm, both_beam_kernels):
    from pyctcdecode_amd import build_ctcdecoder

    dec = build_ctcdecoder(LABELS, lm.path)
    xs = _inputs(lm, 12, seed=1)
    hot = lm.hotwords(5, 1)
    shared = dec.decode_beams_batch(None, xs, beam_width=16, hotwords=hot, hotword_weight=6.0)
    per = dec.decode_beams_batch(None, xs, beam_width=16, hotwords=[list(hot) for _ in xs], hotword_weight=[6.0] * len(xs))
    assert [_key(b) for b in per] == [_key(b) for b in shared]
    assert dec.decode_batch(None, xs, beam_width=16, hotwords=[hot] * len(xs)) == dec.decode_batch(None, xs, beam_width=16, hotwords=hot)


def test_device_fp16_and_multi_lm_inputs(lm, both_beam_kernels):
    from pyctcdecode_amd import build_ctcdecoder
    from pyctcdecode_amd.decoder import BeamSearchDecoderCTC
    from pyctcdecode_amd.alphabet import Alphabet
    from pyctcdecode_amd.language_model import LanguageModel, MultiLanguageModel, NgramModel

    xs = _inputs(lm, 10, seed=2)[2:]
    hot, wts = _hot_lists(lm, len(xs))
    hot = hot[1:] + hot[:1]
    dec = build_ctcdecoder(LABELS, lm.path)
    want = [_key(dec.decode_beams(x, beam_width=16, hotwords=h, hotword_weight=w)) for x, h, w in zip(xs, hot, wts)]
    # host numpy / device tensors
    for inp in (xs, [torch.from_numpy(x).cuda() for x in xs]):
        got = dec.decode_beams_batch(None, inp, beam_width=16, hotwords=hot, hotword_weight=wts)
        assert [_key(g) for g in got] == want
    # fp16 device logits against fp16 single calls
    h16 = [torch.from_numpy(x).cuda().half() for x in xs]
    got = dec.decode_beams_batch(None, h16, beam_width=16, hotwords=hot, hotword_weight=wts)
    assert [_key(g) for g in got] == [_key(dec.decode_beams(x, beam_width=16, hotwords=h, hotword_weight=w))
                                       for x, h, w in zip(h16, hot, wts)]
    # MultiLanguageModel (the workgroup kernel's MULTI variant)
    lm2 = synth.SynthLM(LM_DIR, 200, 300, order=3, seed=5)
    models = [LanguageModel(NgramModel(m.path)) for m in (lm, lm2)]
    multi = BeamSearchDecoderCTC(Alphabet.build_alphabet(LABELS), MultiLanguageModel(models))
    got = multi.decode_beams_batch(None, xs, beam_width=16, hotwords=hot, hotword_weight=wts)
    assert [_key(g) for g in got] == [_key(multi.decode_beams(x, beam_width=16, hotwords=h, hotword_weight=w))
                                       for x, h, w in zip(xs, hot, wts)]


def test_placement_follows_the_utterance(lm):
    from pyctcdecode_amd import build_ctcdecoder

    dec = build_ctcdecoder(LABELS, lm.path)
    n = 1100
    rng = np.random.default_rng(3)
    base = [synth.d_words(2, u, 50, LABELS, False, lm.words, lm.sentences, 28, boost=4.0) for u in range(24)]
    xs = [base[u % 24] for u in range(n)]
    words = list(lm.words)
    hot = [[words[int(i)] for i in rng.choice(len(words), size=3, replace=False)] + ["w%d" % u] for u in range(n)]
    wts = [float(1 + u % 13) for u in range(n)]
    got = dec.decode_beams_batch(None, xs, beam_width=16, hotwords=hot, hotword_weight=wts)
    for u in rng.choice(n, size=16, replace=False):
        u = int(u)
        assert _key(got[u]) == _key(dec.decode_beams(xs[u], beam_width=16, hotwords=hot[u], hotword_weight=wts[u])), u
    rev = dec.decode_beams_batch(None, xs[::-1], beam_width=16, hotwords=hot[::-1], hotword_weight=wts[::-1])
    assert [_key(b) for b in rev] == [_key(b) for b in got[::-1]]


def test_streams_with_per_stream_scorers(lm):
    from pyctcdecode_amd import build_ctcdecoder
    from pyctcdecode_amd.language_model import HotwordScorer

    dec = build_ctcdecoder(LABELS, lm.path)
    n = 4
    xs = [synth.d_words(2, 40 + u, 90, LABELS, False, lm.words, lm.sentences, 28, boost=6.0).astype(np.float64) for u in range(n)]
    cuts = [0, 30, 60, 90]
    sc = [HotwordScorer.build_scorer(lm.hotwords(4, 1, seed=s), weight=w) for s, w in ((1, 8.0), (2, 3.0), (3, 0.0))]
    # per chunk and stream: the scorer (None = no hot words); the scorers change between chunks
    plan = [[sc[0], None, sc[1], sc[2]], [sc[1], sc[0], sc[1], None], [sc[2], sc[0], None, sc[1]]]
    kw = {"beam_width": 16, "prune_history": True}

    def run_alone(u, edit_at=None):
        beams, c1, c2 = dec.get_starting_state()
        for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            if edit_at == k:
                beams = _edited(list(beams), u)
            beams = dec.partial_decode_beams(xs[u][a:b], c1, c2, beams, a, is_end=(b == 90), hotword_scorer=plan[k][u], **kw)
        return beams, c1

    def _edited(beams, u):
        # a list the caller built (the host import): the best beams with a word of this stream's own next scorer in the text
        from pyctcdecode_amd.decoder import Beam

        own = plan[1][u]
        word = own.unigrams[0] if own is not None else "qq"
        out = []
        for b in beams[:5]:
            text = (b.text + " " + word).strip()
            out.append(Beam(text, b.next_word, b.partial_word, b.last_char, list(b.text_frames), b.partial_frames, b.logit_score))
        return out

    alone = [_key(run_alone(u)[0]) for u in range(n)]
    states = [dec.get_starting_state() for _ in range(n)]
    beams_list = [s[0] for s in states]
    for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        beams_list = dec.partial_decode_beams_batch([x[a:b] for x in xs], [s[1] for s in states], [s[2] for s in states],
                                                    beams_list, [a] * n, hotword_scorer=plan[k], is_end=(b == 90), **kw)
    assert [_key(bs) for bs in beams_list] == alone
    # edited host beams after the first chunk (build_import counts each stream's words against its own set)
    alone_e = [_key(run_alone(u, edit_at=1)[0]) for u in range(n)]
    states = [dec.get_starting_state() for _ in range(n)]
    beams_list = [s[0] for s in states]
    for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        if k == 1:
            beams_list = [_edited(list(bs), u) for u, bs in enumerate(beams_list)]
        beams_list = dec.partial_decode_beams_batch([x[a:b] for x in xs], [s[1] for s in states], [s[2] for s in states],
                                                    beams_list, [a] * n, hotword_scorer=plan[k], is_end=(b == 90), **kw)
    assert [_key(bs) for bs in beams_list] == alone_e


def test_device_pool_per_utterance_lists(lm):
    from pyctcdecode_amd import build_ctcdecoder
    from pyctcdecode_amd.parallel import DevicePool

    dec = build_ctcdecoder(LABELS, lm.path)
    xs = [synth.d_words(2, u, t, LABELS, False, lm.words, lm.sentences, 28, boost=4.0) for u, t in enumerate([60, 9, 33, 21, 80, 44])]
    hot, wts = _hot_lists(lm, len(xs))
    want = dec.decode_beams_batch(None, xs, beam_width=16, hotwords=hot, hotword_weight=wts)
    with DevicePool(dec, devices=[0, 0]) as pool:
        got = dec.decode_beams_batch(pool, xs, beam_width=16, hotwords=hot, hotword_weight=wts)
        texts = dec.decode_batch(pool, xs, beam_width=16, hotwords=hot, hotword_weight=wts)
    assert [_key(g) for g in got] == [_key(w) for w in want]
    assert texts == dec.decode_batch(None, xs, beam_width=16, hotwords=hot, hotword_weight=wts)
