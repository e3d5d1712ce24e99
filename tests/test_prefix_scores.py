"""CTC prefix scores (prefix_scores / prefix_scores_batch) on the CPU simulator of the kernels, which runs the bodies of
ctc_forward with end states and of ctc_prefix_extend (csrc/ctc_align.h) itself with a one-thread context: the numpy
definition against the enumeration of all paths, the library against the numpy definition, logp_end equal to score's float,
the chain identity next(g)[c] = lse(end(g + c), next(g + c)), the edge cases, batches equal to single calls bit for bit
(split and unsplit launches among them), and the refusals. The HIP build: tests/test_gpu_prefix_scores.py."""
import ctypes as C
import math

import numpy as np
import pytest

from tests.align_util import random_logits, random_target
from tests.prefix_util import (PREFIX_FUSE_BLOCKS, PREFIX_K, SCORE_TOL, check_prefix, feasible, lse, next_array, prefix_bruteforce,
                               prefix_of_lp, same_prefix)
from tests.score_util import case_input, neg_inf_case, shape_cases
from tests.sim_util import sim_library  # noqa: F401
from tests.test_align import build, ragged_batch

SHAPES = shape_cases()
BLANK = 0  # of tests/align_util.char_labels
ERR_ARG, ERR_LIMIT = -1, -4  # CTCDEC_ERR_ARG, CTCDEC_ERR_LIMIT of include/ctcdec.h


def same(x):
    return x


# ---- the definition against the enumeration -----------------------------------------------------------------------------
ENUM_PREFIXES = ([], [1], [2], [1, 1], [1, 2], [2, 1, 2], [1, 1, 2], [2, 2, 2])


@pytest.mark.parametrize("V,T", ((3, 5), (4, 6)))
@pytest.mark.parametrize("normalised", (True, False), ids=("rows_sum_to_1", "rows_do_not"))
def test_definition_against_enumeration(V, T, normalised):
    assert V ** T <= 4096
    rng = np.random.default_rng(100 * V + T)
    if normalised:
        x = rng.standard_normal((T, V))
        lp = x - np.log(np.exp(x).sum(axis=1, keepdims=True))
    else:
        lp = np.log(rng.uniform(0.05, 0.9, size=(T, V)))  # (any positive matrix: the recursion does not ask for rows that sum to 1)
    for prefix in ENUM_PREFIXES:
        if max(prefix, default=0) >= V:
            continue
        end, nxt = prefix_of_lp(lp, prefix, BLANK)
        want_end, want_next = prefix_bruteforce(lp, prefix, BLANK)
        assert np.array_equal(np.isneginf(nxt), np.isneginf(want_next)), (prefix, nxt, want_next)
        fin = np.isfinite(want_next)
        worst = float(np.abs(nxt[fin] - want_next[fin]).max()) if fin.any() else 0.0
        print("V=%d T=%d prefix %s: end %.12f / %.12f, next worst %.3e" % (V, T, prefix, end, want_end, worst))
        assert worst <= 1e-10 and (end == want_end if math.isinf(want_end) else abs(end - want_end) <= 1e-10)
        if normalised:  # the mass of everything that starts with prefix + [c] is at most the prefix' own
            assert np.exp(nxt[fin]).sum() <= 1.0 + 1e-12


# ---- the library against the definition, and logp_end against score --------------------------------------------------------
def run_shape_case(case, put=same):
    name, V, T, target, _dtype, _kind = case
    dec = build(V)
    x = case_input(case)
    xin = put(x)
    r = dec.prefix_scores(xin, tokens=[target])[0]
    s = dec.score(xin, tokens=[target])[0]
    assert r.logp_end == s.logp, (name, r.logp_end, s.logp)
    assert sum(dec.last_prefix_launched) == (1 if T > 0 else 0)
    check_prefix(r, x, target, BLANK, name)
    return [r]


@pytest.mark.parametrize("case", SHAPES, ids=[c[0] for c in SHAPES])
def test_shape_cases(case, sim_library):  # noqa: F811
    run_shape_case(case)


def run_score_identity(put=same, V=29):
    """Every prefix of every target of the ragged batch, as one call: logp_end is score's float."""
    dec = build(V)
    xs, targets = ragged_batch(n=12, V=V)
    prefixes = [[t[:k] for k in range(0, len(t) + 1, 3)] + [t] for t in targets]
    xin = [put(x) for x in xs]
    got = dec.prefix_scores_batch(xin, tokens=prefixes)
    want = dec.score_batch(xin, tokens=prefixes)
    out = []
    for u, (x, ps) in enumerate(zip(xs, prefixes)):
        for p, g, w in zip(ps, got[u], want[u]):
            assert g.logp_end == w.logp and g.text == w.text, (u, p, g.logp_end, w.logp)
            check_prefix(g, x, p, BLANK, "utt %d, %d labels" % (u, len(p)))
            out.append(g)
    return out


def test_logp_end_is_score(sim_library):  # noqa: F811
    run_score_identity()


def run_chain_identity(put=same, V=7, T=14):
    """next(g)[c] = lse(end(g + c), next(g + c)[.]) on normalised rows: float64 logits at scale 3, no clip active."""
    dec = build(V)
    rng = np.random.default_rng(31)
    x = random_logits(rng, T, V, np.float64, scale=3.0)
    xin = put(x)
    out = []
    for g in ([], [3], [3, 3], random_target(rng, 5, V, doubled=1)):
        assert len(g) in (0, 1, 2, 5)
        longer = [g + [c] for c in range(1, V)]
        base = dec.prefix_scores(xin, tokens=[g])[0]
        ext = dec.prefix_scores(xin, tokens=longer)
        nxt = next_array(base)
        for c, e in zip(range(1, V), ext):
            want = lse([e.logp_end] + next_array(e).tolist())
            print("g=%s c=%d: next %.12f, chain %.12f" % (g, c, nxt[c], want))
            assert abs(nxt[c] - want) <= SCORE_TOL, (g, c, nxt[c], want)
        out += [base] + ext
    return out


def test_chain_identity(sim_library):  # noqa: F811
    run_chain_identity()


# ---- edge cases ------------------------------------------------------------------------------------------------------------
def run_edge_cases(put=same, V=29):
    dec = build(V)
    rng = np.random.default_rng(12)
    out = []
    # one frame: the empty prefix may be followed by any label at frame 0; a one-label prefix is complete and nothing follows
    x1 = random_logits(rng, 1, V)
    got = dec.prefix_scores(put(x1), tokens=[[], [4], [4, 5]])
    assert np.isfinite(next_array(got[0])[1:]).all() and np.isneginf(next_array(got[1])).all()
    assert math.isfinite(got[1].logp_end) and got[2].logp_end == -np.inf and np.isneginf(next_array(got[2])).all()
    assert dec.last_prefix_launched == (2, 0)  # (the prefix without a path launches nothing)
    for p, g in zip(([], [4], [4, 5]), got):
        check_prefix(g, x1, p, BLANK, "T=1 %s" % p)
    out += got
    # exactly as many frames as labels plus repeats: a finite end, nothing can follow; one frame fewer: nothing at all
    hello = [9, 6, 13, 13, 16]
    x6, x5 = random_logits(rng, 6, V), random_logits(rng, 5, V)
    assert feasible(6, hello) and not feasible(5, hello)
    at, below = dec.prefix_scores(put(x6), tokens=[hello])[0], dec.prefix_scores(put(x5), tokens=[hello])[0]
    assert math.isfinite(at.logp_end) and np.isneginf(next_array(at)).all()
    assert below.logp_end == -np.inf and np.isneginf(next_array(below)).all() and dec.last_prefix_launched == (0, 0)
    check_prefix(at, x6, hello, BLANK, "T == L + repeats")
    check_prefix(below, x5, hello, BLANK, "T < L + repeats")
    out += [at, below]
    # no frames
    got = dec.prefix_scores(put(np.zeros((0, V))), tokens=[[], [4]])
    assert got[0].logp_end == 0.0 and got[1].logp_end == -np.inf and all(np.isneginf(next_array(g)).all() for g in got)
    assert next_array(got[0]).shape == (V,) and dec.last_prefix_launched == (0, 0)
    out += got
    # a row of NaN and -inf alone, and -inf at labels of the prefix: the floor
    xn, target = neg_inf_case()
    xn = xn.copy()
    xn[7, :] = np.nan
    xn[7, ::2] = -np.inf
    for p in ([], target[:3], target):
        g = dec.prefix_scores(put(xn), tokens=[p])[0]
        assert math.isfinite(g.logp_end)
        check_prefix(g, xn, p, BLANK, "floor %d" % len(p))
        out.append(g)
    # a prefix whose last label repeats: the column of that label takes the blank-ended weights
    x = random_logits(rng, 20, V)
    for p in ([5, 5], [3, 5, 5, 5], [5]):
        g = dec.prefix_scores(put(x), tokens=[p])[0]
        check_prefix(g, x, p, BLANK, "last label repeats %s" % p)
        out.append(g)
    return out


def test_edge_cases(sim_library):  # noqa: F811
    run_edge_cases()


def mixed_inputs(V, dtype=np.float64, frames=(9, 30, 17, 1)):
    """Probabilities and logits, alternating"""
    rng = np.random.default_rng(V)
    xs = []
    for u, T in enumerate(frames):
        x = random_logits(rng, T, V)
        if u % 2 == 0:
            e = np.exp(x - x.max(axis=1, keepdims=True))
            x = e / e.sum(axis=1, keepdims=True)
        xs.append(x.astype(dtype))
    return xs


def run_batch_equals_single_calls(put=same, xs=None, V=29, per_utt=3):
    """A batch gives the bits of single calls, whatever else is in it."""
    dec = build(V)
    rng = np.random.default_rng(V + 1)
    xs = mixed_inputs(V) if xs is None else xs
    prefixes = [[random_target(rng, int(rng.integers(1, 6)), V, doubled=0) for _ in range(per_utt)] + [[]] for _ in xs]
    xin = [put(x) for x in xs]
    batch = dec.prefix_scores_batch(xin, tokens=prefixes)
    out = []
    for u, (x, ps) in enumerate(zip(xs, prefixes)):
        single = dec.prefix_scores(xin[u], tokens=ps)
        for p, b, s in zip(ps, batch[u], single):
            one = dec.prefix_scores(xin[u], tokens=[p])[0]
            assert same_prefix(b, s) and same_prefix(b, one), (u, p)
            check_prefix(b, x, p, BLANK, "utt %d %s" % (u, p))
            out.append(b)
    return out


def test_batch_equals_single_calls(sim_library):  # noqa: F811
    run_batch_equals_single_calls()


def run_chunks_of_k(put=same, V=29, T=2 * 128 + 1, counts=(PREFIX_K, PREFIX_K + 1)):
    """K and K + 1 prefixes of one utterance -- one full chunk; a full one and one of a single prefix -- give the bits of
    one prefix at a time."""
    dec = build(V)
    rng = np.random.default_rng(77)
    x = random_logits(rng, T, V)
    xin = put(x)
    pool = [random_target(rng, 1 + k % 4, V) for k in range(max(counts))]
    alone = [dec.prefix_scores(xin, tokens=[p])[0] for p in pool]
    for p, a in zip(pool[:3], alone):
        check_prefix(a, x, p, BLANK, "alone %s" % p)
    for n in counts:
        got = dec.prefix_scores(xin, tokens=pool[:n])
        assert len(got) == n and all(same_prefix(g, a) for g, a in zip(got, alone)), n
    return alone


def test_k_and_k_plus_1_prefixes(sim_library):  # noqa: F811
    run_chunks_of_k(T=30)


def run_split_equals_unsplit(put=same, V=29, T=7):
    """A launch of PREFIX_FUSE_BLOCKS chunks runs every segment in one workgroup, a smaller one splits them over workgroups
    and adds their sums afterwards: the same additions in the same order, so the same bits."""
    dec = build(V)
    rng = np.random.default_rng(5)
    x = random_logits(rng, T, V)
    xin = put(x)
    tiles = (V + 255) // 256
    n = -(-PREFIX_FUSE_BLOCKS // tiles) * PREFIX_K
    pool = [[], [3], [3, 3], [4, 9], [9, 4, 9]]
    many = dec.prefix_scores(xin, tokens=[pool[k % len(pool)] for k in range(n)])
    few = dec.prefix_scores(xin, tokens=pool)
    for k in list(range(len(pool))) + [n - 1, n // 2]:
        assert same_prefix(many[k], few[k % len(pool)]), k
    return few


def test_split_and_unsplit_launches(sim_library):  # noqa: F811
    few = run_split_equals_unsplit()
    assert len(few) == 5


def test_two_segments_on_the_simulator(sim_library):  # noqa: F811
    """More frames than a segment holds: the segments' sums are added in order."""
    dec = build(5)
    rng = np.random.default_rng(2)
    x = random_logits(rng, 128 + 3, 5)
    for p in ([], [2, 3, 2]):
        check_prefix(dec.prefix_scores(x, tokens=[p])[0], x, p, BLANK, "two segments %s" % p)


# ---- the Python surface ------------------------------------------------------------------------------------------------------
def test_trailing_space_rule(sim_library):  # noqa: F811
    dec = build(29)
    lab = dec._alphabet.labels
    ids = lambda s: [lab.index(ch) for ch in s]  # noqa: E731
    x = random_logits(np.random.default_rng(4), 30, 29)
    got = dec.prefix_scores(x, texts=["bugs", "bugs ", "  bugs \n ", " bugs   bun", "", "   "])
    assert [g.tokens for g in got] == [ids("bugs"), ids("bugs "), ids("bugs "), ids("bugs bun"), [], []]
    assert [g.text for g in got] == ["bugs", "bugs ", "bugs ", "bugs bun", "", ""]
    assert not same_prefix(got[0], got[1]) and same_prefix(got[1], got[2])
    by_tokens = dec.prefix_scores(x, tokens=[g.tokens for g in got])
    assert all(same_prefix(a, b) for a, b in zip(got, by_tokens))
    assert dec._target_of_text("bugs ") == ids("bugs")  # (the targets of the other calls keep their rule)
    assert isinstance(got[0].next_logp, np.ndarray) and dec.last_prefix_next is None
    assert len(dec.last_prefix_timing_ms) == 5 and dec.last_prefix_launched == (6, 0)


def test_refusals(sim_library):  # noqa: F811
    from pyctcdecode_amd import _binding as B
    from pyctcdecode_amd import build_ctcdecoder, parallel
    from pyctcdecode_amd.parallel import DevicePool
    from tests.test_greedy import BPE_PIECES

    dec = build(29)
    x = random_logits(np.random.default_rng(1), 10, 29)
    for bad in (BLANK, 29, -1, 2.0, True):
        with pytest.raises(ValueError, match="utterance 1, prefix 2"):
            dec.prefix_scores_batch([x, x], tokens=[[[2]], [[2], [3], [4, bad]]])
    with pytest.raises(ValueError, match="utterance 0 got a bare str"):
        dec.prefix_scores_batch([x], texts=["bugs"])
    with pytest.raises(ValueError, match="bare str"):
        dec.prefix_scores(x, texts="bugs")
    for kwargs in ({}, {"texts": ["a"], "tokens": [[2]]}):
        with pytest.raises(ValueError, match="exactly one of texts and tokens"):
            dec.prefix_scores(x, **kwargs)
    with pytest.raises(ValueError, match="utterance 0, prefix 1 is not a str"):
        dec.prefix_scores(x, texts=["a", 3])
    with pytest.raises(ValueError, match="not a label of the alphabet"):
        dec.prefix_scores(x, texts=["bügs"])
    with pytest.raises(ValueError, match="utterance 0, prefix 1 has 2048 labels, above the limit of 2047"):
        dec.prefix_scores(x, tokens=[[2], [2, 3] * 1024])
    with pytest.raises(ValueError, match="prefixes for 2 utterances"):
        dec.prefix_scores_batch([x], tokens=[[[2]], [[3]]])
    bpe = build_ctcdecoder(BPE_PIECES)
    xb = random_logits(np.random.default_rng(1), 10, len(bpe._alphabet.labels))
    with pytest.raises(ValueError, match="BPE"):
        bpe.prefix_scores(xb, texts=["bugs"])
    assert len(bpe.prefix_scores(xb, tokens=[[1, 2], []])) == 2
    pool = object.__new__(DevicePool)  # (no workers started: the refusal comes first)
    with pytest.raises(NotImplementedError):
        pool.prefix_scores_batch([x], tokens=[[[2]]])
    with pytest.raises(NotImplementedError):
        pool.prefix_scores(x, tokens=[[2]])
    with pytest.raises(NotImplementedError):
        parallel.prefix_scores_batch_sharded(dec, [x], tokens=[[[2]]])
    # the C entry point: everything is checked before anything moves
    dll, h = sim_library.dll, dec._handle
    ptrs = np.array([x.ctypes.data], dtype=np.uint64)
    frames = np.array([10], dtype=np.int32)

    def call(labels, label_off, prefix_off, kernel=0, frames=frames, next_out=None):
        labels, res = np.asarray(labels, dtype=np.int32), C.c_void_p()
        rc = dll.ctcdec_prefix_batch(h, ptrs.ctypes.data_as(C.POINTER(C.c_void_p)), frames.ctypes.data_as(C.POINTER(C.c_int32)), 1, 1, 0,
                                     labels.ctypes.data_as(C.POINTER(C.c_int32)), B.off_ptr(np.asarray(label_off, dtype=np.int64)),
                                     B.off_ptr(np.asarray(prefix_off, dtype=np.int64)), kernel, next_out, C.byref(res))
        if rc == 0:
            dll.ctcdec_prefix_free(res)
        return rc

    assert call([2, 3], [0, 2], [0, 1]) == 0
    for bad in ([BLANK, 3], [2, 29], [2, -1]):
        assert call(bad, [0, 2], [0, 1]) == ERR_ARG
        assert "utterance 0, prefix 0" in dll.ctcdec_last_error().decode()
    assert call([2, 3], [1, 2], [0, 1]) == ERR_ARG and call([2, 3], [0, 2, 1], [0, 2]) == ERR_ARG
    assert call([2, 3], [0, 2], [1, 1]) == ERR_ARG and call([2, 3], [0, 2], [0, 1], kernel=3) == ERR_ARG
    assert call([2, 3], [0, 2], [0, 1], frames=np.array([-1], dtype=np.int32)) == ERR_ARG
    assert call([2] * 2048, [0, 2048], [0, 1]) == ERR_LIMIT
    room = np.zeros(29)
    assert call([2, 3], [0, 2], [0, 1], next_out=C.c_void_p(room.ctypes.data)) == ERR_ARG  # (a buffer for next is device memory)


def test_forward_kernel_env(sim_library, monkeypatch):  # noqa: F811
    dec = build(29)
    x = random_logits(np.random.default_rng(3), 12, 29)
    plain = dec.prefix_scores(x, tokens=[[2, 3]])[0]
    monkeypatch.setenv("CTCDEC_FORWARD_KERNEL", "group")
    forced = dec.prefix_scores(x, tokens=[[2, 3]])[0]
    assert dec.last_prefix_launched == (0, 1) and same_prefix(plain, forced)
    monkeypatch.setenv("CTCDEC_FORWARD_KERNEL", "fast")
    with pytest.raises(ValueError, match="CTCDEC_FORWARD_KERNEL"):
        dec.prefix_scores(x, tokens=[[2, 3]])
