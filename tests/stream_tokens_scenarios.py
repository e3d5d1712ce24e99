"""Scenarios of streaming token frames and confidences (partial_decode_beams(..., token_frames=True / confidence=...), DESIGN.md
"Streaming tokens and confidences"), shared by tests/test_stream_tokens.py (CPU, the simulator build) and
tests/test_gpu_stream_tokens.py (-m gpu). Inputs are those of tests/test_resident_streams.py: synth.d_words, T = 180, cuts
[0, 50, 51, 120, 180] (a one-frame chunk, tokens across the cuts; CUTS_OF), the 28-label character alphabet and the 255-piece BPE
vocabulary, the 4-gram synthetic LM, prune_history=True. `build` is build_ctcdecoder, `to_input(chunk)` hands a numpy chunk to
the decoder (as it is, or as a device tensor)."""
import ctypes as C

import numpy as np
import pytest

import synth
from oracle.ctc_oracle import build_oracle
from pyctcdecode_amd.alphabet import Alphabet
from tests.golden_util import check_beams
from tests.test_resident_streams import BPE, LM, _lm_beams, _oracle_beams, _oracle_chunks
from tests.token_frames_util import check_tokens, clean
from tests.token_logp_util import FOLDS, LOGP_FLOOR, check_token_logp, lp_matrix, tol_of

T = 180
# The character alphabet's best beam holds ('n', (50, 52)) on this input: the cut at 51 runs through it. On the BPE vocabulary
# no token of the best beam lies across 50 / 51 / 120, so its cuts are moved onto ('n', (51, 54)) and ('s', (122, 124)): the
# one-frame chunk [52, 53) then lies wholly inside a token.
CUTS_OF = {False: [0, 50, 51, 120, 180], True: [0, 52, 53, 123, 180]}
ALPHABETS = [(40, synth.LIBRI_LABELS, False), (100, BPE, True)]
ALPHABET_IDS = ["chars-40", "bpe-100"]


def make_input(labels, is_bpe, seed=5, dtype=np.float64):
    return synth.d_words(3, seed, T, labels, is_bpe, LM.words, LM.sentences, len(labels), boost=6.0).astype(dtype)


def stream(dec, x, to_input, cuts, first=0, on_chunk=None, **kw):
    """Feed x in chunks, handing every list back unread; on_chunk(k, beams) may look. -> (end beams, the lists seen)"""
    beams, c1, c2 = dec.get_starting_state()
    seen = []
    for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        beams = dec.partial_decode_beams(to_input(x[a:b]), c1, c2, beams, first + a, is_end=(b == cuts[-1]), prune_history=True, **kw)
        seen.append(beams)
        if on_chunk is not None:
            on_chunk(k, beams)
    return beams, seen


def words_of(b):
    return list(zip(b.text.split(), list(b.text_frames)))


def split_open(b):
    """(tokens of the closed words, tokens of the open partial word)"""
    toks = list(b.token_frames)
    if not b.partial_word:
        return toks, []
    k = len(toks)
    while k > 0 and toks[k - 1][1][0] >= b.partial_frames[0]:
        k -= 1
    return toks[:k], toks[k:]


def check_stream_beams(beams, labels, is_bpe, lp, fold=None, tol=None, what=""):
    """Every property of a list of TokenLMBeams / ConfidenceLMBeams; -> all tokens checked, as (start, end)."""
    spans = []
    for i, b in enumerate(beams):
        w = "%s beam %d" % (what, i)
        closed, opened = split_open(b)
        check_tokens(words_of(b), closed, labels, is_bpe, lp, what=w)
        if b.partial_word:
            assert opened, w
            assert "".join(clean(t[0], is_bpe) for t in opened) == b.partial_word, (w, opened, b.partial_word)
            assert opened[0][1][0] == b.partial_frames[0] and opened[-1][1][1] == b.partial_frames[1], (w, opened, b.partial_frames)
            for (_l, (s, e)), (_l2, (s2, _e2)) in zip(opened, opened[1:]):
                assert s < e <= s2, (w, opened)
        else:
            assert not opened
        if fold is not None:
            check_token_logp(b.token_frames, b.token_logp, labels, lp, fold, tol, w)
            assert len(b.word_logp) == len(b.text_frames), w
            for (word, (ws, we)), got in zip(words_of(b), b.word_logp):
                run = [v for (_lab, (s, e)), v in zip(closed, b.token_logp) if ws <= s and e <= we]
                assert run and got == min(run) and LOGP_FLOOR <= got <= 0.0, (w, word, got, run)
        spans += [t[1] for t in b.token_frames]
    return spans


def key_of(b):
    return (b.text, b.partial_word, list(b.text_frames), b.partial_frames, b.logit_score, b.lm_score, list(b.token_frames),
            list(getattr(b, "token_logp", [])), list(getattr(b, "word_logp", [])))


def scenario_unread_then_end(build, to_input, beam_width, labels, is_bpe, dtype=np.float64):
    """1 + 2: nothing is built until the end; the end is the oracle's chunked decode (float64) with tokens and confidences that
    hold against the whole matrix; tokens do run across the cuts."""
    from pyctcdecode_amd import ConfidenceLMBeam
    from pyctcdecode_amd.decoder import _ResidentBeams

    dec = build(labels, LM.path)
    alphabet = Alphabet.build_alphabet(labels)
    x = make_input(labels, is_bpe, dtype=dtype)
    lp = lp_matrix(x)
    ends = {}
    CUTS = CUTS_OF[is_bpe]
    for fold in FOLDS:
        beams, seen = stream(dec, x, to_input, CUTS, beam_width=beam_width, confidence=fold)
        assert all(isinstance(s, _ResidentBeams) and not s._filled for s in seen[:-1])  # never looked at, never built
        assert beams and all(type(b) is ConfidenceLMBeam for b in beams) and all(b.partial_word == "" for b in beams)
        spans = check_stream_beams(beams, alphabet.labels, is_bpe, lp, fold, tol_of(dtype), "%s end" % fold)
        ends[fold] = beams
        # straddling is really exercised: a token across a cut, and a token that ended before the last chunk began
        assert any(s < cut < e for (s, e) in spans for cut in CUTS[1:-1]), "no token runs across a cut"
        assert any(e <= CUTS[-2] for (_s, e) in spans)
    assert [key_of(b)[:7] for b in ends["mean"]] == [key_of(b)[:7] for b in ends["min"]] == [key_of(b)[:7] for b in ends["max"]]
    if dtype == np.float64:  # the flags change nothing else: text, frames and scores are the oracle's chunked decode
        orc = build_oracle(alphabet.labels, alphabet.is_bpe, LM.path, None)
        exp = _oracle_chunks(orc, x, CUTS, beam_width=beam_width, prune_history=True)
        check_beams(_lm_beams(ends["mean"]), _oracle_beams(exp), what="stream tokens, unread chunks")
    return dec, x, ends


def scenario_chunking_changes_nothing(build, to_input, beam_width, labels, is_bpe):
    """3: one chunk, five chunks and the one-shot decode give the same float64 per token, compared with ==."""
    dec = build(labels, LM.path)
    x = make_input(labels, is_bpe)
    for fold in FOLDS:
        five, _ = stream(dec, x, to_input, CUTS_OF[is_bpe], beam_width=beam_width, confidence=fold)
        one, _ = stream(dec, x, to_input, [0, T], beam_width=beam_width, confidence=fold)
        whole = dec.decode_beams(to_input(x), beam_width=beam_width, prune_history=True, confidence=fold)
        n = 0
        for a, b, w in zip(five, one, whole):
            if a.text == b.text and a.token_frames == b.token_frames:
                assert a.token_logp == b.token_logp and a.word_logp == b.word_logp, (fold, a.text)
                if w.text == a.text and w.token_frames == a.token_frames:
                    assert w.token_logp == a.token_logp and w.word_logp == a.word_logp, (fold, a.text)
                    n += 1
        assert five[0].text == one[0].text == whole[0].text and five[0].token_frames == one[0].token_frames == whole[0].token_frames
        assert n >= 1 and five[0].token_logp == whole[0].token_logp


def scenario_mid_stream_reads(build, to_input, beam_width, labels, is_bpe, fold="mean"):
    """4: beams[0] after chunk 2 (the cheap read), the full list after chunk 3; closed words, then the open word; handing the
    read lists back continues the stream to the same end."""
    from pyctcdecode_amd import ConfidenceLMBeam
    from pyctcdecode_amd.decoder import _ResidentBeams

    dec = build(labels, LM.path)
    alphabet = Alphabet.build_alphabet(labels)
    x = make_input(labels, is_bpe)
    lp = lp_matrix(x)
    CUTS = CUTS_OF[is_bpe]
    want, _ = stream(dec, x, to_input, CUTS, beam_width=beam_width, confidence=fold)
    looked = {}

    def look(k, beams):
        if k == 1:
            best = beams[0]
            assert isinstance(beams, _ResidentBeams) and not beams._filled and type(best) is ConfidenceLMBeam
            looked["best"] = check_stream_beams([best], alphabet.labels, is_bpe, lp[:CUTS[2]], fold, tol_of(x.dtype), "best after chunk 2")
            rest = list(beams)  # ... and then the whole list of the same chunk: the same first beam
            assert key_of(rest[0]) == key_of(best)
            looked["open"] = any(b.partial_word for b in rest)
            check_stream_beams(rest, alphabet.labels, is_bpe, lp[:CUTS[2]], fold, tol_of(x.dtype), "all after chunk 2")
        elif k == 2:
            full = list(beams)
            assert full and all(type(b) is ConfidenceLMBeam for b in full)
            looked["full"] = check_stream_beams(full, alphabet.labels, is_bpe, lp[:CUTS[3]], fold, tol_of(x.dtype), "all after chunk 3")
            looked["open"] = looked["open"] or any(b.partial_word for b in full)
            # a token that lies wholly in an earlier chunk than the one that returned it, and one across a cut
            assert any(e <= CUTS[2] for (_s, e) in looked["full"]) and any(s < c < e for (s, e) in looked["full"] for c in CUTS[1:3])

    got, _ = stream(dec, x, to_input, CUTS, beam_width=beam_width, confidence=fold, on_chunk=look)
    assert looked["best"] and looked["full"] and looked["open"], "no read saw the tokens of an open word"
    assert [key_of(b) for b in got] == [key_of(b) for b in want]


def scenario_batch_of_streams(build, to_input, beam_width):
    """5: three streams with different chunk lengths per call, one of them a single frame: each ends as it does alone."""
    labels, is_bpe = BPE, True
    dec = build(labels, LM.path)
    alphabet = Alphabet.build_alphabet(labels)
    xs = [make_input(labels, is_bpe, seed=5 + u) for u in range(3)]
    cuts = [CUTS_OF[True], [0, 1, 90, 150, T], [0, 60, 100, 101, T]]
    states = [dec.get_starting_state() for _ in xs]
    beams = [s[0] for s in states]
    for k in range(4):
        beams = dec.partial_decode_beams_batch([to_input(x[c[k]:c[k + 1]]) for x, c in zip(xs, cuts)], [s[1] for s in states],
                                               [s[2] for s in states], beams, [c[k] for c in cuts], beam_width=beam_width,
                                               prune_history=True, is_end=(k == 3), confidence="mean")
    for u, x in enumerate(xs):
        alone, _ = stream(dec, x, to_input, cuts[u], beam_width=beam_width, confidence="mean")
        assert [key_of(b) for b in beams[u]] == [key_of(b) for b in alone], u
        check_stream_beams(beams[u], alphabet.labels, is_bpe, lp_matrix(x), "mean", tol_of(x.dtype), "stream %d" % u)


def scenario_force_next_word(build, to_input, beam_width, labels, is_bpe, fold="min"):
    """6: force_next_word=True on a middle chunk closes the open word there; the tokens follow. The cuts are the plain ones for
    both alphabets: a forced boundary resets last_char (decoder.py:693-728), so one that falls INSIDE a run of a label splits
    it into two tokens of that label without a gap -- the reference's own rule, and not what check_tokens' gap property is about."""
    dec = build(labels, LM.path)
    alphabet = Alphabet.build_alphabet(labels)
    x = make_input(labels, is_bpe)
    lp = lp_matrix(x)
    CUTS = CUTS_OF[False]
    beams, c1, c2 = dec.get_starting_state()
    n_forced = 0
    for k, (a, b) in enumerate(zip(CUTS[:-1], CUTS[1:])):
        beams = dec.partial_decode_beams(to_input(x[a:b]), c1, c2, beams, a, beam_width=beam_width, prune_history=True,
                                         force_next_word=(k == 2), is_end=(b == T), confidence=fold)
        if k == 2:
            full = list(beams)
            assert full and all(b_.partial_word == "" for b_ in full)  # every word is closed at this chunk's end
            spans = check_stream_beams(full, alphabet.labels, is_bpe, lp[:b], fold, tol_of(x.dtype), "forced")
            n_forced = len(spans)
            assert max(e for _s, e in spans) <= b
    assert n_forced > 0
    check_stream_beams(beams, alphabet.labels, is_bpe, lp, fold, tol_of(x.dtype), "after force_next_word")


def scenario_probabilities(build, to_input, beam_width, labels, is_bpe):
    """7: probability-like chunks (softmax rows as float32): the fold is checked against lp_matrix of each chunk."""
    dec = build(labels, LM.path)
    alphabet = Alphabet.build_alphabet(labels)
    z = make_input(labels, is_bpe)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    p = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    CUTS = CUTS_OF[is_bpe]
    lp = np.concatenate([lp_matrix(p[a:b]) for a, b in zip(CUTS[:-1], CUTS[1:])])
    for a, b in zip(CUTS[:-1], CUTS[1:]):  # (every chunk is read as probabilities: its own rows sum to 1 in float32)
        assert np.isclose(float(p[a:b].sum(axis=1).mean()), 1.0)
    for fold in FOLDS:
        beams, _ = stream(dec, p, to_input, CUTS, beam_width=beam_width, confidence=fold)
        spans = check_stream_beams(beams, alphabet.labels, is_bpe, lp, fold, tol_of(np.float32), "probabilities %s" % fold)
        assert spans


def scenario_refusals(build, to_input, monkeypatch):
    """8: each refusal raises the documented exception and leaves the previous chunk's lists readable."""
    labels = synth.LIBRI_LABELS
    dec = build(labels, LM.path)
    x = make_input(labels, False)
    kw = dict(beam_width=30, prune_history=True)

    def start(**first):
        beams, c1, c2 = dec.get_starting_state()
        return dec.partial_decode_beams(to_input(x[:50]), c1, c2, beams, 0, **kw, **first), c1, c2

    def still_readable(lazy, token_beams):
        assert len(lazy) > 0 and lazy[0].text is not None
        assert hasattr(lazy[0], "token_frames") == token_beams

    # a fold first asked for at chunk 2
    lazy, c1, c2 = start()
    with pytest.raises(ValueError):
        dec.partial_decode_beams(to_input(x[50:51]), c1, c2, lazy, 50, confidence="mean", **kw)
    still_readable(lazy, False)
    lazy, c1, c2 = start(token_frames=True)
    with pytest.raises(ValueError):
        dec.partial_decode_beams(to_input(x[50:51]), c1, c2, lazy, 50, confidence="mean", **kw)
    still_readable(lazy, True)
    # a changed fold
    lazy, c1, c2 = start(confidence="mean")
    with pytest.raises(ValueError):
        dec.partial_decode_beams(to_input(x[50:51]), c1, c2, lazy, 50, confidence="min", **kw)
    # a processed_frames that skips ahead
    with pytest.raises(ValueError):
        dec.partial_decode_beams(to_input(x[50:51]), c1, c2, lazy, 60, confidence="mean", **kw)
    with pytest.raises(ValueError):
        dec.partial_decode_beams(to_input(x[50:51]), c1, c2, lazy, 50, confidence="median", **kw)
    still_readable(lazy, True)
    # ... and the stream goes on from there (token_frames alone may be asked of a stream with a fold)
    nxt = dec.partial_decode_beams(to_input(x[50:51]), c1, c2, lazy, 50, token_frames=True, **kw)
    assert type(nxt[0]).__name__ == "TokenLMBeam"
    end = dec.partial_decode_beams(to_input(x[51:]), c1, c2, nxt, 51, is_end=True, confidence="mean", **kw)
    assert type(end[0]).__name__ == "ConfidenceLMBeam"
    # edited beams
    lazy, c1, c2 = start(token_frames=True)
    edited = list(lazy)[:3]
    with pytest.raises(NotImplementedError, match="built or edited"):
        dec.partial_decode_beams(to_input(x[50:51]), c1, c2, edited, 50, token_frames=True, **kw)
    still_readable(lazy, True)
    # a seeded memo
    beams, c1, c2 = dec.get_starting_state()
    c1[("", False)] = (0.0, 0.0, dec.decode_beams(to_input(x[:40]))[0].last_lm_state)
    with pytest.raises(NotImplementedError, match="seeded"):
        dec.partial_decode_beams(to_input(x[:50]), c1, c2, beams, 0, confidence="mean", **kw)
    # a changed hot-word set forces an import
    from pyctcdecode_amd.language_model import HotwordScorer

    lazy, c1, c2 = start(token_frames=True)
    with pytest.raises(NotImplementedError, match="hot words"):
        dec.partial_decode_beams(to_input(x[50:51]), c1, c2, lazy, 50, token_frames=True,
                                 hotword_scorer=HotwordScorer.build_scorer(LM.hotwords(4, 1), weight=8.0), **kw)
    still_readable(lazy, True)
    # CTCDEC_RESIDENT_STREAMS=0
    monkeypatch.setenv("CTCDEC_RESIDENT_STREAMS", "0")
    beams, c1, c2 = dec.get_starting_state()
    with pytest.raises(NotImplementedError, match="CTCDEC_RESIDENT_STREAMS"):
        dec.partial_decode_beams(to_input(x[:50]), c1, c2, beams, 0, token_frames=True, **kw)
    monkeypatch.delenv("CTCDEC_RESIDENT_STREAMS")
    # the library's own refusals (the shell raises before it gets there): a fold the first push did not ask for, a changed
    # one, a first_frame that skips ahead -- CTCDEC_ERR_ARG each, and the stream stays where it was
    from pyctcdecode_amd import _binding as B

    lazy, c1, c2 = start(confidence="max")
    st = lazy._streams
    chunk = np.ascontiguousarray(x[50:51])
    ptrs, frames = (C.c_void_p * 1)(chunk.ctypes.data), (C.c_int32 * 1)(1)
    for token_frames, ff in ((2, 50), (4, 60)):
        p = B.Params.from_buffer_copy(st.params)
        p.token_frames = token_frames
        res = C.c_void_p()
        rc = st.lib.dll.ctcdec_stream_push(st.handle, ptrs, frames, 1, 0, C.byref(p), (C.c_int32 * 1)(ff), 0, 0, 1, C.byref(res))
        assert rc == -1, (token_frames, ff, rc)
    got = (C.c_int64 * 1)()
    st.lib.check(st.lib.dll.ctcdec_stream_frames(st.handle, got))
    assert got[0] == 50
    still_readable(lazy, True)


def scenario_nothing_for_those_who_do_not_ask(build, to_input, beam_width, labels, is_bpe):
    """9: without the arguments a stream returns plain LMBeams, today's, and its handle holds no ledger."""
    from pyctcdecode_amd.decoder import LMBeam

    def ledger_bytes(lazy):
        st = lazy._streams
        n = (C.c_int64 * 1)()
        st.lib.check(st.lib.dll.ctcdec_stream_ledger_bytes(st.handle, n))
        return int(n[0])

    dec = build(labels, LM.path)
    alphabet = Alphabet.build_alphabet(labels)
    orc = build_oracle(alphabet.labels, alphabet.is_bpe, LM.path, None)
    x = make_input(labels, is_bpe)
    CUTS = CUTS_OF[is_bpe]
    held = []
    beams, seen = stream(dec, x, to_input, CUTS, beam_width=beam_width, on_chunk=lambda k, b: held.append(ledger_bytes(b)) if k < 3 else None)
    assert held == [0, 0, 0]
    assert all(type(b) is LMBeam for b in beams)
    check_beams(_lm_beams(beams), _oracle_beams(_oracle_chunks(orc, x, CUTS, beam_width=beam_width, prune_history=True)), what="plain")
    held = []
    stream(dec, x, to_input, CUTS, beam_width=beam_width, token_frames=True, on_chunk=lambda k, b: held.append(ledger_bytes(b)) if k < 3 else None)
    assert held == [0, 0, 0]  # (token frames alone come from the chains)
    held = []
    conf, _ = stream(dec, x, to_input, CUTS, beam_width=beam_width, confidence="mean",
                     on_chunk=lambda k, b: held.append(ledger_bytes(b)) if k < 3 else None)
    assert all(h > 0 for h in held)
    # a compact ledger: far below what max_surv entries per frame would take (150 x 10 bytes x 180 frames = 270 kB)
    assert max(held) < 150 * 10 * T
    plain = lambda b: (b.text, b.partial_word, list(b.text_frames), b.partial_frames, b.logit_score, b.lm_score)  # noqa: E731
    assert [plain(b) for b in conf] == [plain(b) for b in beams]
