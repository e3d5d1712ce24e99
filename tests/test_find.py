"""Phrase search (find / find_batch) on the CPU simulator of the kernels, which runs the body of ctc_find (csrc/ctc_align.h)
itself with a one-thread context: the shape cases of tests/align_util.py with a label to search for, each in its own matrix,
against the numpy recursion and selection of tests/find_util.py; utterances too short for the phrase; planted occurrences with
max_hits below, at and above their number; min_logp; one-label phrases; batches equal to single calls float for float, in one
launch and in several; text against tokens; -inf logits; and the refusals of the Python surface and of the C entry point.
The HIP build: tests/test_gpu_find.py."""
import math

import numpy as np
import pytest

from tests.find_util import (MAX_HITS, SCORE_TOL, case_input, check_found, feasible, neg_inf_case, planted_input, random_logits,
                             random_target, shape_cases, windows_of, yardstick)
from tests.sim_util import sim_library  # noqa: F401
from tests.test_align import build
from tests.token_logp_util import lp_matrix

SHAPES = [c for c in shape_cases() if len(c[3]) >= 1]
WHOLE_MATRIX = ("T1_L1", "T_eq_L_no_blanks", "hello_at_bound", "aaa_at_bound")  # as many frames as the phrase needs: one window
# (occurrences planted, max_hits): below, at and above their number
PLANTED = [(1, 1), (1, 3), (2, 1), (2, 2), (2, 4), (3, 2), (3, 3), (3, 5)]


def same(a, b):
    """Two PhraseSearch results float for float, window for window, and frame for frame of their traces."""
    if (a.text, a.tokens, a.hits) != (b.text, b.tokens, b.hits) or (a.end_logp is None) != (b.end_logp is None):
        return False
    return a.end_logp is None or (np.array_equal(a.end_logp, b.end_logp) and np.array_equal(a.end_start, b.end_start))


def planted_case(n_occ, seed=0, L=4, V=29, T=90, dtype=np.float64):
    """(x, phrase, windows): `n_occ` occurrences of a phrase of L labels (one doubled) in T frames of unit-normal noise."""
    rng = np.random.default_rng(100 * n_occ + seed)
    phrase = random_target(rng, L, V, doubled=1 if L > 1 else 0)
    starts = [(7, 40, 66)[k] + int(rng.integers(0, 5)) for k in range(n_occ)]
    x, windows = planted_input(rng, T, V, phrase, 0, starts, dtype)
    return x, phrase, windows


@pytest.mark.parametrize("case", SHAPES, ids=[c[0] for c in SHAPES])
def test_shape_cases(case, sim_library):  # noqa: F811
    name, V, T, target, _dtype, _kind = case
    dec = build(V)
    x = case_input(case)
    blank = dec._alphabet.labels.index("")
    got = dec.find(x, tokens=[target], max_hits=3, trace=True)
    assert len(got) == 1 and dec.last_find_launched in ((1, 0), (0, 1)) and dec.last_find_launches == 1
    assert dec.last_find_launched == ((1, 0) if len(target) <= 127 else (0, 1))
    check_found(got[0], x, target, blank, max_hits=3, what=name)
    assert len(got[0].hits) >= 1
    if name in WHOLE_MATRIX:
        assert windows_of(got[0]) == [(0, T)], (name, got[0].hits)
        assert abs(got[0].hits[0].logp - dec.align(x, tokens=target).score) <= SCORE_TOL
    plain = dec.find(x, tokens=[target], max_hits=3)[0]
    assert plain.end_logp is None and plain.hits == got[0].hits


def test_no_frames_and_too_few_frames(sim_library):  # noqa: F811
    dec = build(29)
    got = dec.find(np.zeros((0, 29)), tokens=[[2, 3], [4]], max_hits=2, trace=True)
    assert [g.hits for g in got] == [[], []] and dec.last_find_launched == (0, 0) and dec.last_find_launches == 0
    assert all(g.end_logp.shape == (0,) and g.end_start.shape == (0,) for g in got)
    rng = np.random.default_rng(3)
    for target, T in (([9, 6, 13, 13, 16], 6), ([2, 2, 2], 5)):
        assert feasible(T, target) and not feasible(T - 1, target)
        short = random_logits(rng, T - 1, 29)
        got = dec.find(short, tokens=[target], trace=True)[0]
        assert got.hits == [] and dec.last_find_launched == (0, 0)
        assert np.all(got.end_logp == -np.inf) and np.all(got.end_start == -1) and got.end_logp.shape == (T - 1,)
        ok = random_logits(rng, T, 29)
        got = dec.find(ok, tokens=[target], max_hits=2)[0]
        assert windows_of(got) == [(0, T)] and dec.last_find_launched == (1, 0)
    # one utterance long enough, one not: only the first takes part in the device work
    xs = [random_logits(rng, 20, 29), random_logits(rng, 3, 29)]
    got = dec.find_batch(xs, tokens=[[[2, 3, 4, 5]], [[2, 3, 4, 5]]])
    assert len(got[0][0].hits) == 1 and got[1][0].hits == [] and dec.last_find_launched == (1, 0)
    assert same(got[0][0], dec.find(xs[0], tokens=[[2, 3, 4, 5]])[0])


@pytest.mark.parametrize("n_occ,max_hits", PLANTED, ids=["%d_planted_%d_hits" % c for c in PLANTED])
def test_planted_phrases(n_occ, max_hits, sim_library):  # noqa: F811
    dec = build(29)
    x, phrase, windows = planted_case(n_occ)
    got = dec.find(x, tokens=[phrase], max_hits=max_hits, trace=True)[0]
    ref = check_found(got, x, phrase, 0, max_hits=max_hits, what="%d planted, max_hits %d" % (n_occ, max_hits))
    want = yardstick(x, phrase, 0, max_hits)[0]
    assert windows_of(got) == [(s, e) for s, e, _ in want]  # (a margin of nats: the windows themselves)
    first = windows_of(got)[:n_occ]
    assert set(first) <= set(windows) and len(first) == min(n_occ, max_hits), (first, windows)
    if max_hits > n_occ:
        assert len(got.hits) > n_occ
        print("the hit after the planted ones lies %.2f nats below them" % (got.hits[n_occ - 1].logp - got.hits[n_occ].logp))
        assert got.hits[n_occ].logp < got.hits[n_occ - 1].logp
    assert np.array_equal(got.end_start, ref[1])  # (and every end frame's window)


def test_min_logp_cuts_the_list(sim_library):  # noqa: F811
    dec = build(29)
    x, phrase, windows = planted_case(2, seed=1)
    everything = dec.find(x, tokens=[phrase], max_hits=6)[0]
    assert len(everything.hits) > 2
    # a threshold between the planted occurrences and the best of the rest
    floor = (everything.hits[1].logp + everything.hits[2].logp) / 2
    got = dec.find(x, tokens=[phrase], max_hits=6, min_logp=floor, trace=True)[0]
    check_found(got, x, phrase, 0, max_hits=6, min_logp=floor, what="min_logp")
    assert sorted(windows_of(got)) == sorted(windows) and got.hits == everything.hits[:2]
    assert [(s, e) for s, e, _ in yardstick(x, phrase, 0, 6, floor)[0]] == windows_of(got)
    # the threshold itself qualifies, nothing above the best does
    at = dec.find(x, tokens=[phrase], max_hits=6, min_logp=everything.hits[1].logp)[0]
    assert at.hits == everything.hits[:2]
    assert dec.find(x, tokens=[phrase], max_hits=6, min_logp=np.nextafter(everything.hits[0].logp, 1.0))[0].hits == []
    assert dec.find(x, tokens=[phrase], min_logp=math.inf)[0].hits == []
    assert dec.find(x, tokens=[phrase], max_hits=6, min_logp=-math.inf)[0].hits == everything.hits


def test_one_label_phrases_are_single_frames(sim_library):  # noqa: F811
    dec = build(29)
    rng = np.random.default_rng(11)
    x = random_logits(rng, 23, 29)
    lp = lp_matrix(x)
    got = dec.find(x, tokens=[[7]], max_hits=MAX_HITS, trace=True)[0]
    check_found(got, x, [7], 0, max_hits=MAX_HITS, what="L=1")
    assert len(got.hits) == 23 and all(h.frames == 1 for h in got.hits)
    assert [h.start for h in got.hits] == np.argsort(-lp[:, 7], kind="stable").tolist()
    assert np.array_equal(got.end_start, np.arange(23))
    assert max(abs(h.logp - lp[h.start, 7]) for h in got.hits) <= SCORE_TOL
    top = dec.find(x, tokens=[[7]], max_hits=5)[0]
    assert top.hits == got.hits[:5]


def ragged_phrases(seed=4, V=29, dtype=np.float64):
    """Utterances with 0, 1 and 5 phrases each -- one of them too long for its utterance, one above the wave kernel's length."""
    rng = np.random.default_rng(seed)
    xs, phrases = [], []
    for u, (T, count) in enumerate(((40, 5), (25, 0), (61, 1), (9, 5), (300, 1), (33, 1))):
        xs.append(random_logits(rng, T, V, dtype))
        cur = [random_target(rng, int(rng.integers(1, 9)), V) for _ in range(count)]
        if u == 3:
            cur[2] = random_target(rng, 12, V)  # (12 labels, 9 frames)
        if u == 4:
            cur[0] = random_target(rng, 130, V, doubled=3)
        phrases.append(cur)
    return xs, phrases


def test_batch_equals_single_calls(sim_library):  # noqa: F811
    dec = build(29)
    xs, phrases = ragged_phrases()
    batch = dec.find_batch(xs, tokens=phrases, max_hits=3, trace=True)
    n_launched = sum(1 for x, cur in zip(xs, phrases) for p in cur if feasible(len(x), p))
    assert sum(dec.last_find_launched) == n_launched == 12 and dec.last_find_launched[1] == 1 and dec.last_find_launches == 2
    assert [len(b) for b in batch] == [5, 0, 1, 5, 1, 1]
    for u, (x, cur) in enumerate(zip(xs, phrases)):
        singles = dec.find(x, tokens=cur, max_hits=3, trace=True)
        for j, p in enumerate(cur):
            assert same(batch[u][j], singles[j]), (u, j)
            assert same(batch[u][j], dec.find(x, tokens=[p], max_hits=3, trace=True)[0]), (u, j)
            check_found(batch[u][j], x, p, 0, max_hits=3, what="utt %d phrase %d" % (u, j))
    assert batch[3][2].hits == []
    # several launches: a budget of 12 * 61 bytes holds the trace of one phrase of the 61-frame utterance, or a few shorter ones
    split = dec.find_batch(xs, tokens=phrases, max_hits=3, trace=True, _trace_budget=12 * 300)
    assert dec.last_find_launches > 2 and sum(dec.last_find_launched) == 12
    assert all(same(a, b) for cur_a, cur_b in zip(batch, split) for a, b in zip(cur_a, cur_b))
    with pytest.raises(ValueError, match="utterance 4, phrase 0.*budget"):
        dec.find_batch(xs, tokens=phrases, _trace_budget=12 * 300 - 1)
    # padded into one [B, T, V] array, and the phrases from generators
    T = max(len(x) for x in xs)
    pad = np.zeros((len(xs), T, 29))
    for u, x in enumerate(xs):
        pad[u, : len(x)] = x
    cube = dec.find_batch(pad, tokens=(iter(cur) for cur in phrases), max_hits=2)
    for u, cur in enumerate(phrases):
        assert [g.hits for g in cube[u]] == [g.hits for g in dec.find(pad[u], tokens=cur, max_hits=2)], u
    assert dec.find_batch([], []) == [] and dec.find(xs[0], []) == [] and dec.last_find_launched == (0, 0)


def test_text_and_tokens_give_the_same_result(sim_library):  # noqa: F811
    dec = build(29)
    labels = dec._alphabet.labels
    rng = np.random.default_rng(8)
    target = [labels.index(c) for c in "bugs bunny"]
    x, windows = planted_input(rng, 70, 29, target, 0, [21])
    texts = ["  bugs   bunny \n", "bug", "y"]
    toks = [[labels.index(c) for c in " ".join(t.split())] for t in texts]
    a, b = dec.find(x, texts, max_hits=2, trace=True), dec.find(x, tokens=toks, max_hits=2, trace=True)
    assert all(same(p, q) for p, q in zip(a, b)) and [g.tokens for g in a] == toks
    assert [g.text for g in a] == ["bugs bunny", "bug", "y"]
    assert windows_of(a[0])[0] == windows[0] and a[1].hits[0].start == 21 and a[1].hits[0].end == 21 + 5
    assert same(a[0], dec.find_batch([x, x], [["bug"], ["bugs bunny"]], max_hits=2, trace=True)[1][0])


def test_neg_inf_logits(sim_library):  # noqa: F811
    dec = build(29)
    x, phrase = neg_inf_case()
    assert np.isneginf(x[:, phrase]).any()
    got = dec.find(x, tokens=[phrase], max_hits=3, trace=True)[0]
    assert got.hits and all(math.isfinite(h.logp) for h in got.hits)
    check_found(got, x, phrase, 0, max_hits=3, what="-inf logits")


def test_bad_arguments(sim_library, monkeypatch):  # noqa: F811
    from pyctcdecode_amd import build_ctcdecoder
    from pyctcdecode_amd.decoder import _ResidentBeams

    dec = build(5)
    labels = dec._alphabet.labels
    x = np.zeros((9, 5))
    with pytest.raises(ValueError, match="utterance 0.*bare str"):
        dec.find(x, "ab")
    with pytest.raises(ValueError, match="utterance 1.*bare str"):
        dec.find_batch([x, x], [["ab"], "ab"])
    with pytest.raises(ValueError, match="2 utterances"):
        dec.find_batch([x, x], [["a"]])
    with pytest.raises(ValueError, match="utterances"):
        dec.find_batch([x], "a")
    for bad in ([labels.index("")], [5], [-1], [2.0], [True]):
        with pytest.raises(ValueError, match="utterance 0, phrase 1.*label id"):
            dec.find(x, tokens=[[2], bad])
    with pytest.raises(ValueError, match="utterance 0, phrase 0.*limit of 2047"):
        dec.find(np.zeros((2100, 5)), tokens=[random_target(np.random.default_rng(1), 2048, 5)])
    with pytest.raises(ValueError, match="utterance 0, phrase 1 is empty"):
        dec.find(x, tokens=[[2], []])
    with pytest.raises(ValueError, match="utterance 1, phrase 0 is empty"):
        dec.find_batch([x, x], [["a"], ["  "]])
    with pytest.raises(ValueError, match="utterance 0, phrase 0 is not a str"):
        dec.find(x, [[2, 3]])
    with pytest.raises(ValueError, match="utterance 0, phrase 0 is a str"):
        dec.find(x, tokens=["ab"])
    for bad in (0, 65, -1, 2.5, True, None):
        with pytest.raises(ValueError, match="max_hits"):
            dec.find(x, ["ab"], max_hits=bad)
    with pytest.raises(ValueError, match="min_logp"):
        dec.find(x, ["ab"], min_logp=float("nan"))
    with pytest.raises(ValueError, match="'z'"):
        dec.find(x, ["ab z"])
    with pytest.raises(ValueError, match="exactly one"):
        dec.find(x, ["ab"], tokens=[[2, 3]])
    with pytest.raises(ValueError, match="exactly one"):
        dec.find_batch([x])
    with pytest.raises(ValueError):
        dec.find(np.zeros((9, 6)), ["ab"])
    with pytest.raises(ValueError, match="utterance 0, phrase 0.*budget"):
        dec.find_batch([x], [["ab"]], _trace_budget=12 * 9 - 1)
    monkeypatch.setenv("CTCDEC_FIND_KERNEL", "warp")
    with pytest.raises(ValueError, match="CTCDEC_FIND_KERNEL"):
        dec.find(x, ["ab"])
    monkeypatch.delenv("CTCDEC_FIND_KERNEL")
    with pytest.raises(NotImplementedError, match="stream"):
        dec.find(_ResidentBeams.__new__(_ResidentBeams), ["ab"])
    with pytest.raises(NotImplementedError, match="stream"):
        dec.find_batch([_ResidentBeams.__new__(_ResidentBeams)], [["ab"]])
    assert len(dec.find(x, ["ab"])[0].hits) == 1  # (the decoder still works)
    bpe = build_ctcdecoder(["<unk>", "▁bug", "s", "▁bun", "ny", "▁", "n", "▁a"])
    xb = random_logits(np.random.default_rng(4), 25, len(bpe._alphabet.labels))
    with pytest.raises(ValueError, match="tokens="):
        bpe.find(xb, ["bugs bunny"])
    lab = bpe._alphabet.labels
    target = [lab.index(p) for p in ("▁bug", "s", "▁bun", "n", "n", "ny", "▁a")]
    got = bpe.find(xb, tokens=[target], max_hits=2)[0]
    assert got.text == "bugs bunnnny a"
    check_found(got, xb, target, lab.index(""), max_hits=2, what="bpe")


def test_native_call_validates_what_it_indexes_with(sim_library):  # noqa: F811
    """The C entry point on its own: null pointers, decreasing offsets, a label outside the alphabet, the blank, an empty
    phrase, max_hits outside 1 .. 64, a NaN min_logp, too many labels and a trace above the budget are error codes before
    anything is launched, and the process lives."""
    import ctypes as C

    dec = build(5)
    blank = dec._alphabet.labels.index("")
    x = np.random.default_rng(2).standard_normal((6, 5))
    I32, I64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    dll = dec._lib.dll

    def call(phrases, loff=None, hoff=None, frames=6, null=(), kernel=0, max_hits=2, min_logp=-math.inf, trace=0, budget=0):
        ptrs = (C.c_void_p * 1)(None if "x" in null else x.ctypes.data)
        fr = (C.c_int32 * 1)(frames)
        flat = np.array([c for t in phrases for c in t] or [0], dtype=np.int32)
        lo = np.array(loff if loff is not None else np.concatenate(([0], np.cumsum([len(t) for t in phrases]))), dtype=np.int64)
        ho = np.array(hoff if hoff is not None else [0, len(phrases)], dtype=np.int64)
        res = C.c_void_p()
        rc = dll.ctcdec_find_batch(
            None if "dec" in null else dec._handle, None if "ptrs" in null else ptrs, None if "frames" in null else fr, 1, 1, 0,
            None if "hoff" in null else ho.ctypes.data_as(I64), None if "loff" in null else lo.ctypes.data_as(I64),
            None if "labels" in null else flat.ctypes.data_as(I32), max_hits, min_logp, trace, kernel, budget,
            None if "out" in null else C.byref(res))
        counts = None
        if rc == 0:
            ho_, ps, pe, pl, n = C.POINTER(C.c_int64)(), I32(), I32(), C.POINTER(C.c_double)(), C.c_int64()
            assert dll.ctcdec_search_hits(res, C.byref(ho_), C.byref(ps), C.byref(pe), C.byref(pl), C.byref(n)) == 0
            assert n.value == len(phrases)
            counts = np.diff(np.ctypeslib.as_array(ho_, shape=(len(phrases) + 1,))).tolist()
            to, tl, ts = C.POINTER(C.c_int64)(), C.POINTER(C.c_double)(), I32()
            assert dll.ctcdec_search_trace(res, C.byref(to), C.byref(tl), C.byref(ts)) == 0
            assert bool(tl) == bool(trace) and bool(ts) == bool(trace)
            assert dll.ctcdec_search_hits(res, None, C.byref(ps), C.byref(pe), C.byref(pl), C.byref(n)) == -1
            assert dll.ctcdec_search_trace(None, C.byref(to), C.byref(tl), C.byref(ts)) == -1
            assert dll.ctcdec_search_timing(res, None, None, None) == -1
            dll.ctcdec_search_free(res)
        return rc, counts

    assert call([[2, 3], [2, 2, 2, 2], [4]]) == (0, [2, 0, 2])
    assert call([[2, 3]], trace=1) == (0, [2]) and call([[2, 3]], kernel=1)[0] == 0 and call([[2, 3]], kernel=2)[0] == 0
    for what in ("dec", "ptrs", "frames", "labels", "loff", "hoff", "out", "x"):
        assert call([[2, 3]], null=(what,))[0] == -1, what
    assert call([[2, 5]])[0] == -1 and call([[2], [-1]])[0] == -1 and call([[blank]])[0] == -1
    assert call([[2, 3]], loff=[0, -1])[0] == -1 and call([[2, 3]], loff=[1, 2])[0] == -1
    assert call([[2], [3]], loff=[0, 2, 1])[0] == -1
    assert call([[2, 3]], hoff=[0, -1])[0] == -1 and call([[2, 3]], hoff=[1, 1])[0] == -1
    assert call([[2, 3]], frames=-1)[0] == -1 and call([[2, 3]], kernel=3)[0] == -1
    assert call([[2, 3], []])[0] == -1  # (an empty phrase)
    assert call([[2, 3]], max_hits=0)[0] == -1 and call([[2, 3]], max_hits=65)[0] == -1 and call([[2, 3]], max_hits=64)[0] == 0
    assert call([[2, 3]], min_logp=float("nan"))[0] == -1 and call([[2, 3]], min_logp=math.inf) == (0, [0])
    assert call([[2, 3]], budget=-1)[0] == -1
    assert call([[2] * 2048])[0] == -4
    assert call([[2, 3]], budget=12 * 6 - 1)[0] == -4 and call([[2, 3]], budget=12 * 6)[0] == 0
    assert call([[2, 3]]) == (0, [2])  # (the decoder still works)


def test_parallel_refuses(sim_library):  # noqa: F811
    from pyctcdecode_amd.parallel import DevicePool, find_batch_sharded

    dec = build(5)
    with pytest.raises(NotImplementedError):
        find_batch_sharded(dec, [np.zeros((3, 5))], [["a"]])
    with DevicePool(dec, devices=[0], library=sim_library.path) as pool:
        with pytest.raises(NotImplementedError):
            pool.find_batch([np.zeros((3, 5))], [["a"]])
        with pytest.raises(NotImplementedError):
            pool.find(np.zeros((3, 5)), ["a"])
