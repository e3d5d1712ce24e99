"""Phrase spotting on streams (spot_streams / SpotStreams.feed; DESIGN.md "Phrase spotting on streams") for the CPU and GPU
tests: the cases, the cuts into chunks, a stream fed chunk by chunk and put together again as the PhraseSpot that spot_batch
returns for the whole recording, and the checks both suites run."""
import numpy as np
import pytest

from pyctcdecode_amd import PhraseSpot
from tests.spot_util import check_spot, random_logits, random_target, same
from tests.test_align import build

LENGTHS = (1, 2, 15, 16, 31, 32, 63, 64, 127)  # the segment widths' borders, and the phrase whose one lane owns both ends
CUTS = ("ones", "ragged", "whole")


def length_case(L):
    """(phrase, x): 40 frames where the phrase fits them, about 300 otherwise; the phrase once, +10 along its tightest path"""
    rng = np.random.default_rng(5000 + L)
    phrase = random_target(rng, L, 29, doubled=min(2, L // 2))
    need = L + sum(1 for a, b in zip(phrase, phrase[1:]) if a == b)
    T = 40 if need <= 33 else max(300, need + 7)
    x = random_logits(rng, T, 29)
    t = (T - need) // 2
    for k, c in enumerate(phrase):
        t += k > 0 and phrase[k - 1] == c
        x[t, c] += 10.0
        t += 1
    return phrase, x


def cut(T, name):
    """Chunk lengths that add up to T: all ones; 1, 7, 0, 64 and the rest (which may be empty); the whole at once"""
    if name == "ones":
        return [1] * T
    sizes = []
    for n in ((1, 7, 0, 64) if name == "ragged" else ()):
        sizes.append(min(n, T - sum(sizes)))
    return sizes + [T - sum(sizes)]


def feed_all(session, rows, sizes_per_stream, to_input, after=None):
    """Feed stream u its chunks sizes_per_stream[u] of rows[u], the last with is_end (streams with fewer chunks get empty ones
    afterwards); check first_frame and the entries' number call by call. -> per stream, per phrase (end_logp, end_start, count)"""
    n, feeds = len(rows), max(len(s) for s in sizes_per_stream)
    at, parts, count = [0] * n, None, None
    for k in range(feeds):
        sizes = [s[k] if k < len(s) else 0 for s in sizes_per_stream]
        ends = [k == len(s) - 1 for s in sizes_per_stream]
        got = session.feed([to_input(r[a:a + m]) for r, a, m in zip(rows, at, sizes)], is_end=ends)
        if after:
            after(k)
        parts = parts or [[([], []) for _ in cur] for cur in got]
        for u, cur in enumerate(got):
            before, over = at[u], k >= len(sizes_per_stream[u])
            final_before = before if over else max(before - 1, 0)
            final_after = before + sizes[u] if ends[u] or over else max(before + sizes[u] - 1, 0)
            for j, c in enumerate(cur):
                assert c.first_frame == final_before and len(c.end_logp) == len(c.end_start) == final_after - final_before, (k, u, j)
                parts[u][j][0].append(c.end_logp)
                parts[u][j][1].append(c.end_start)
            at[u] += sizes[u]
        count = [[c.count for c in cur] for cur in got]
    return [[(np.concatenate(p[0]), np.concatenate(p[1]), count[u][j]) for j, p in enumerate(cur)] for u, cur in enumerate(parts)]


def stream_spots(dec, rows, phrases, sizes_per_stream, to_input=lambda x: x, max_hits=3, after=None):
    """The streams fed chunk by chunk, as what spot_batch(..., trace=True) returns for the whole recordings"""
    with dec.spot_streams(tokens=phrases, max_frames=max(len(r) for r in rows) or 1) as s:
        traces = feed_all(s, rows, sizes_per_stream, to_input, after)
        hits = s.hits(max_hits=max_hits)
        texts = s._texts
    return [[PhraseSpot(texts[u][j], list(p), hits[u][j], t[2], t[0], t[1].astype(np.int32)) for j, (p, t) in enumerate(zip(cur, traces[u]))]
            for u, cur in enumerate(phrases)]


def check_chunked_equals_whole(L, name, to_input=lambda x: x):
    """Any cut gives the whole recording's trace, count and hits float for float, and both lie within SCORE_TOL of numpy"""
    phrase, x = length_case(L)
    dec = build(29)
    whole = dec.spot(to_input(x), tokens=[phrase], max_hits=3, trace=True)[0]
    got = stream_spots(dec, [x], [[phrase]], [cut(len(x), name)], to_input)[0][0]
    assert np.array_equal(got.end_logp, whole.end_logp) and np.array_equal(got.end_start, whole.end_start), (L, name)
    assert same(got, whole), (L, name, got.count, whole.count, got.hits, whole.hits)
    check_spot(got, x, phrase, 0, max_hits=3, what="L=%d %s" % (L, name))
    return got


def packing_case():
    """3 streams of 50, 23 and 0 frames: 9 phrases of at most 15 labels on the first (a second wavefront of 8 lanes an item),
    one phrase of every width on the second, which ends a feed earlier; the third never gets a frame."""
    rng = np.random.default_rng(77)
    rows = [random_logits(rng, 50, 29), random_logits(rng, 23, 29), np.zeros((0, 29))]
    phrases = [[random_target(rng, L, 29) for L in (1, 2, 3, 5, 8, 8, 13, 15, 15)],
               [random_target(rng, L, 29, doubled=1) for L in (3, 20, 40, 100)], [random_target(rng, 4, 29)]]
    return rows, phrases, [[20, 30], [23], [0, 0]]


def check_packing(monkeypatch, to_input=lambda x: x):
    rows, phrases, sizes = packing_case()
    dec = build(29)
    whole = dec.spot_batch([to_input(r) for r in rows], tokens=phrases, max_hits=3, trace=True)
    got = {}
    for width, waves in (("", [(2, 1, 1, 1), (2, 0, 0, 0)]), ("64", [(0, 0, 0, 13), (0, 0, 0, 9)])):
        monkeypatch.setenv("CTCDEC_SPOT_STREAM_WIDTH", width) if width else monkeypatch.delenv("CTCDEC_SPOT_STREAM_WIDTH", raising=False)

        def launched(k, width=width, waves=waves):
            assert dec.last_spot_stream_launched == waves[k] and dec.last_spot_stream_launches == 1, (width, k)

        got[width] = stream_spots(dec, rows, phrases, sizes, to_input, after=launched)
    for u, cur in enumerate(whole):
        for j, w in enumerate(cur):
            assert same(got[""][u][j], got["64"][u][j]) and same(got[""][u][j], w), (u, j)


def check_refusals():
    from pyctcdecode_amd.parallel import DevicePool

    dec = build(29)
    x = random_logits(np.random.default_rng(3), 12, 29)
    with pytest.raises(ValueError, match="spot"):
        dec.spot_streams(tokens=[[[1 + k % 27 for k in range(128)]]])
    with dec.spot_streams(tokens=[[[3, 4]]]) as s:
        with pytest.raises(ValueError, match="max_frames"):
            s.hits()
        s.feed([x[:5]], is_end=True)
        with pytest.raises(ValueError, match="ended"):
            s.feed([x[5:6]])
    want = dec.spot(x[:10], tokens=[[3, 4]], trace=True)[0]
    s = dec.spot_streams(tokens=[[3, 4]], n_streams=1, max_frames=10)
    first = s.feed([x[:6]])[0][0]
    with pytest.raises(ValueError, match="max_frames"):
        s.feed([x[6:11]])
    last = s.feed([x[6:10]], is_end=True)[0][0]  # (the session is as the refused feed found it)
    assert np.array_equal(np.concatenate([first.end_logp, last.end_logp]), want.end_logp) and last.count == want.count
    assert s.hits() == [[want.hits]]
    s.close()
    with pytest.raises(ValueError, match="closed"):
        s.feed([x[:1]])
    with pytest.raises(NotImplementedError):
        DevicePool.spot_streams(None, tokens=[[[3]]])
