"""Prefix sessions (BeamSearchDecoderCTC.prefix_session; DESIGN.md "Prefix sessions"), shared by the CPU and GPU tests: the
runners. The yardstick of every one of them is the stateless call on the same input -- a session's prefix and
prefix_scores_batch(tokens=...) of the same labels are compared with == (tests.prefix_util.same_prefix: logp_end and all of
next_logp) --, and a sample of the session's prefixes also goes through check_prefix against the numpy definition, which
is not this library. ``put`` places a numpy matrix where the test wants it (as it is, or on the device); ``host_of`` gives
back the exact values the library then reads, for the numpy definition."""
import numpy as np
import pytest

from tests.align_util import random_logits
from tests.prefix_util import PREFIX_FUSE_BLOCKS, PREFIX_K, SCORE_TOL, check_prefix, lse, next_array, same_prefix
from tests.test_align import build
from tests.test_prefix_scores import mixed_inputs

BLANK = 0  # of tests/align_util.char_labels
FRAMES = (1, 2, 127, 128, 129, 257)  # around PREFIX_SEG, and the shortest


def same(x):
    return x


def inputs(V, dtype, frames, mixed=True):
    """The batch of a runner: one utterance per frame count -- probabilities and logits alternating, or logits alone"""
    if mixed:
        return mixed_inputs(V, dtype, frames)
    rng = np.random.default_rng(V)
    return [random_logits(rng, T, V).astype(dtype) for T in frames]


def stateless(dec, xin, nodes):
    """prefix_scores_batch of the nodes' labels, in the nodes' order"""
    per_utt = [[] for _ in xin]
    for k, node in enumerate(nodes):
        per_utt[node.utt].append(k)
    got = dec.prefix_scores_batch(xin, tokens=[[nodes[k].tokens for k in ks] for ks in per_utt])
    out = [None] * len(nodes)
    for ks, res in zip(per_utt, got):
        for k, r in zip(ks, res):
            out[k] = r
    return out


def assert_equal_stateless(dec, xin, nodes, what=""):
    want = stateless(dec, xin, nodes)
    for node, w in zip(nodes, want):
        assert same_prefix(node, w), (what, node.utt, node.tokens, node.logp_end, w.logp_end)
    return want


def run_tree_walk(put=same, V=29, dtype=np.float64, frames=FRAMES, depth=12, mixed=True, host_of=None):
    """A random tree per utterance: at every depth one live prefix gets three children -- its last label again, a label that
    differs from it, and a random one --, one of which is walked on from; the others stay live or are released."""
    dec = build(V)
    rng = np.random.default_rng(7 * V + len(frames))
    xs = inputs(V, dtype, frames, mixed)
    xin = [put(x) for x in xs]
    ref = [host_of(t) for t in xin] if host_of else xs
    with dec.prefix_session(xin) as s:
        roots = s.roots
        empty = dec.prefix_scores_batch(xin, tokens=[[[]] for _ in xin])
        assert [r.utt for r in roots] == list(range(len(xs))) and all(r.tokens == [] and r.text == "" for r in roots)
        for r, w in zip(roots, empty):
            assert same_prefix(r, w[0]), (r.utt, r.logp_end, w[0].logp_end)
        nodes, at = list(roots), list(roots)
        for d in range(depth):
            parents, labels = [], []
            for node in at:
                last = node.tokens[-1] if node.tokens else int(rng.integers(1, V))
                other = 1 + (last - 1 + int(rng.integers(1, V - 1))) % (V - 1)
                assert other != last and other != BLANK
                parents += [node.id] * 3
                labels += [last if node.tokens else other, other, int(rng.integers(1, V))]
            kids = s.extend(parents, labels)
            assert len(kids) == len(parents) and s.last_launches[2:] == (0, 0)
            for k, (p, c) in zip(kids, zip(parents, labels)):
                assert k.tokens == s._nodes[p].tokens + [c] and k.utt == s._nodes[p].utt
            nodes += kids
            at = [kids[3 * u + int(rng.integers(0, 3))] for u in range(len(xs))]
            if d % 3 == 2:  # (some leaves go: their slots are reused by the next depth)
                drop = [k for k in kids if k not in at][::2]
                s.release([k.id for k in drop])
        assert_equal_stateless(dec, xin, nodes, "tree V=%d %s" % (V, np.dtype(dtype)))
        for node in nodes[:: max(1, len(nodes) // 24)] + nodes[-3:]:
            check_prefix(node, ref[node.utt], node.tokens, BLANK, "tree utt %d %s" % (node.utt, node.tokens))
    return nodes


def run_forward_boundary(put=same, setenv=None):
    """One chain to 130 labels: the stateless call takes the wave kernel up to 127 labels and the group kernel above, the
    session has one path. At 20 labels both forward kernels are forced."""
    V, T = 7, 300
    dec = build(V)
    rng = np.random.default_rng(130)
    x = random_logits(rng, T, V)
    xin = put(x)
    chain = rng.integers(1, V, size=130).tolist()
    assert len(chain) + sum(1 for a, b in zip(chain, chain[1:]) if a == b) < T
    kept = []
    with dec.prefix_session([xin], capacity=3) as s:
        node = s.roots[0]
        for k, c in enumerate(chain):
            kid = s.extend([node.id], [c])[0]
            if node.tokens:
                s.release([node.id])
            node = kid
            if len(node.tokens) in (20, 126, 127, 128, 129, 130):
                kept.append(node)
    assert [len(k.tokens) for k in kept] == [20, 126, 127, 128, 129, 130]
    for k in kept[1:]:
        w = dec.prefix_scores(xin, tokens=[k.tokens])[0]
        assert dec.last_prefix_launched == ((1, 0) if len(k.tokens) <= 127 else (0, 1))
        assert same_prefix(k, w), (len(k.tokens), k.logp_end, w.logp_end)
    check_prefix(kept[-1], x, kept[-1].tokens, BLANK, "130 labels")
    for kernel, launched in (("wave", (1, 0)), ("group", (0, 1))):
        setenv("CTCDEC_FORWARD_KERNEL", kernel)
        w = dec.prefix_scores(xin, tokens=[kept[0].tokens])[0]
        assert dec.last_prefix_launched == launched and same_prefix(kept[0], w), kernel
    return kept


def run_infeasible(put=same, V=5):
    """Chains longer than the frames allow, with repeated labels: -inf exactly where the stateless call has it, and the
    finite end at T == labels + repeats."""
    dec = build(V)
    rng = np.random.default_rng(3)
    frames = (0, 1, 3, 3)
    xs = [random_logits(rng, T, V) for T in frames]
    xin = [put(x) for x in xs]
    chains = ([2, 2, 3], [2, 2, 3], [2, 2, 3, 3, 4], [2, 3, 4, 4, 2])
    out = []
    with dec.prefix_session(xin) as s:
        at = list(s.roots)
        out += at
        for d in range(5):
            live = [(node, chains[node.utt][d]) for node in at if d < len(chains[node.utt])]
            at = s.extend([node.id for node, _c in live], [c for _node, c in live])
            out += at
        want = assert_equal_stateless(dec, xin, out, "infeasible")
    for node, w in zip(out, want):
        T, need = frames[node.utt], len(node.tokens) + sum(1 for a, b in zip(node.tokens, node.tokens[1:]) if a == b)
        nxt = next_array(node)
        if T < need or T == 0:
            assert node.logp_end == (0.0 if T == 0 and not node.tokens else -np.inf) and np.isneginf(nxt).all(), (T, node.tokens)
        else:
            assert np.isfinite(node.logp_end) and (T > need or np.isneginf(nxt).all()), (T, node.tokens)
        check_prefix(node, xs[node.utt], node.tokens, BLANK, "T=%d %s" % (T, node.tokens))
    assert any(frames[n.utt] == len(n.tokens) + 1 == 3 and np.isfinite(n.logp_end) for n in out)  # ([2, 2]: T == L + repeats)
    return out


def run_independence(put=same, V=29):
    """A child's bits depend on nothing else in the call: another order, one child a call, a session over its utterance
    alone, and PREFIX_K or PREFIX_K + 1 children of one utterance."""
    dec = build(V)
    rng = np.random.default_rng(11)
    xs = mixed_inputs(V, np.float64, frames=(9, 130, 17))
    xin = [put(x) for x in xs]
    with dec.prefix_session(xin) as s:
        first = s.extend([r.id for r in s.roots], [3, 4, 5])
        parents = [first[k % 3] for k in range(3 * (PREFIX_K + 1))]
        labels = [int(c) for c in rng.integers(1, V, size=len(parents))]
        labels[:3] = [3, 9, 5]  # (the first utterance's repeats its last label)
        base = s.extend([p.id for p in parents], labels)
        perm = rng.permutation(len(parents)).tolist()
        shuffled = s.extend([parents[k].id for k in perm], [labels[k] for k in perm])
        for j, k in enumerate(perm):
            assert same_prefix(shuffled[j], base[k]), k
        for k in (0, 1, 2, len(parents) - 1):
            assert same_prefix(s.extend([parents[k].id], [labels[k]])[0], base[k]), k
        # PREFIX_K children of the second utterance fill one chunk, PREFIX_K + 1 need a second
        for count in (PREFIX_K, PREFIX_K + 1):
            got = s.extend([first[1].id] * count, list(range(2, 2 + count)))
            for g, c in zip(got, range(2, 2 + count)):
                assert same_prefix(g, s.extend([first[1].id], [c])[0]), (count, c)
        assert_equal_stateless(dec, xin, base, "independence")
    for u in (0, 1):
        with dec.prefix_session([xin[u]]) as alone:
            kid = alone.extend([alone.roots[0].id], [first[u].tokens[0]])[0]
            mine = [k for k in range(len(parents)) if parents[k].utt == u]
            got = alone.extend([kid.id] * len(mine), [labels[k] for k in mine])
            for g, k in zip(got, mine):
                assert g.utt == 0 and g.tokens == base[k].tokens and g.logp_end == base[k].logp_end
                assert np.array_equal(next_array(g), next_array(base[k])), k
    return base


def run_split_equals_fused(put=same, V=29, T=7):
    """Few children make an extension that is split by segments, PREFIX_FUSE_BLOCKS chunks one that is not."""
    dec = build(V)
    x = random_logits(np.random.default_rng(5), T, V)
    xin = put(x)
    n = -(-PREFIX_FUSE_BLOCKS // ((V + 255) // 256)) * PREFIX_K
    pool = [3, 4, 9, 3, 12]
    with dec.prefix_session([xin], capacity=n + len(pool) + 2) as s:
        mid = s.extend([s.roots[0].id], [3])[0]
        few = s.extend([mid.id] * len(pool), pool)
        few_launches = s.last_launches
        many = s.extend([mid.id] * n, [pool[k % len(pool)] for k in range(n)])
        many_launches = s.last_launches
        for k in list(range(len(pool))) + [n - 1, n // 2]:
            assert same_prefix(many[k], few[k % len(pool)]), k
        assert_equal_stateless(dec, [xin], few, "split")
    return few, few_launches, many_launches


def run_arena(put=same, V=5):
    """The arena fills, refuses, and goes on after a release; a reused slot gives a fresh session's bits; every refusal
    leaves the session usable."""
    dec = build(V)
    rng = np.random.default_rng(9)
    xs = [random_logits(rng, T, V) for T in (6, 4)]
    xin = [put(x) for x in xs]
    with dec.prefix_session(xin, capacity=6) as s, dec.prefix_session(xin, capacity=6) as other:
        a = s.extend([s.roots[0].id, s.roots[1].id, s.roots[0].id], [2, 3, 4])
        b = s.extend([a[0].id], [2])
        assert len(s) == 6 == s.capacity
        with pytest.raises(ValueError, match="slots"):
            s.extend([a[1].id], [2])
        s.release([a[2].id])
        c = s.extend([a[1].id], [2])[0]  # (in the slot that a[2] had)
        fresh = other.extend([other.extend([other.roots[1].id], [3])[0].id], [2])[0]
        assert same_prefix(c, fresh)
        foreign = other.extend([other.roots[0].id], [4])[0]
        for bad_parent in (a[2].id, foreign.id, -1, 1 << 40, "0", None):
            with pytest.raises(ValueError, match="live prefix"):
                s.extend([bad_parent], [2])
        for bad_label in (BLANK, V, -1, 2.0, True):
            with pytest.raises(ValueError, match="labels\\[0\\]"):
                s.extend([a[0].id], [bad_label])
        with pytest.raises(ValueError, match="live prefix"):
            s.release([a[2].id])
        with pytest.raises(ValueError, match="empty prefix"):
            s.release([b[0].id, s.roots[0].id])
        with pytest.raises(ValueError, match="twice"):
            s.release([b[0].id, b[0].id])
        with pytest.raises(ValueError, match="exactly one of labels and texts"):
            s.extend([a[0].id])
        with pytest.raises(ValueError, match="2 labels for 1 parents"):
            s.extend([a[0].id], [2, 3])
        assert len(s) == 6
        s.release([b[0].id])  # (the refusals released nothing and took nothing)
        again = s.extend([a[0].id], [2])[0]
        assert same_prefix(again, b[0]) and again.id != b[0].id
        with pytest.raises(ValueError, match="live prefix"):
            s.extend([b[0].id], [3])  # (the id stays dead although its slot is live again)
        assert_equal_stateless(dec, xin, [a[0], a[1], c, again], "arena")
        s.release([c.id])
        by_text = s.extend([s.roots[0].id], texts=["a"])[0]  # ("a" is label 2 of tests/align_util.char_labels)
        assert by_text.tokens == [2] and by_text.text == "a" and same_prefix(by_text, a[0])
        with pytest.raises(ValueError, match="single character"):
            s.extend([s.roots[0].id], texts=["ab"])
    with pytest.raises(ValueError, match="closed"):
        s.extend([s.roots[0].id], [2])
    with pytest.raises(ValueError, match="closed"):
        s.release([a[0].id])
    s.close()  # (a second close is nothing)
    with pytest.raises(ValueError, match="capacity"):
        dec.prefix_session(xin, capacity=1)


def run_label_limit(put=same):
    """A chain of 2047 labels is the longest: T = 1 and V = 3 leave the kernels nothing to do."""
    dec = build(3)
    xin = put(random_logits(np.random.default_rng(1), 1, 3))
    with dec.prefix_session([xin], capacity=3) as s:
        node = s.roots[0]
        for k in range(2047):
            kid = s.extend([node.id], [1 + k % 2])[0]
            if node.tokens:
                s.release([node.id])
            node = kid
        assert len(node.tokens) == 2047 and node.logp_end == -np.inf
        with pytest.raises(ValueError, match="2048 labels, above the limit of 2047"):
            s.extend([node.id], [1])
        s.release([node.id])
        assert np.isfinite(s.extend([s.roots[0].id], [2])[0].logp_end)


def run_cost_contract(put=same, V=300, T=500):
    """An extend launches ctc_prefix_advance once and neither row_lse nor a forward kernel; its extension launches what
    the stateless call's does for the same prefixes."""
    dec = build(V)
    rng = np.random.default_rng(1)
    xin = put(random_logits(rng, T, V).astype(np.float32))
    with dec.prefix_session([xin]) as s:
        opened = s.last_launches
        kids = s.extend([s.roots[0].id] * 8, [int(c) for c in rng.integers(1, V, size=8)])
        first = s.last_launches
        kids = s.extend([k.id for k in kids], [int(c) for c in rng.integers(1, V, size=8)])
        second, ms = s.last_launches, s.last_timing_ms
        dec.prefix_scores(xin, tokens=[k.tokens for k in kids])
    print("open", opened, "extend", first, second, "ms", ms, "stateless", dec.last_prefix_launches, dec.last_prefix_timing_ms)
    assert first == second and second[0] == 1 and second[2:] == (0, 0)
    assert second[1] == dec.last_prefix_launches[2]
    assert len(ms) == 3 and ms[2] > 0.0
    return opened, second, ms, dec.last_prefix_launches


def run_chain_identity(put=same, V=7, T=14):
    """exp(next(g)[c]) = exp(end(g + c)) + sum exp(next(g + c)[.]) on normalised rows, from a session's own results"""
    dec = build(V)
    rng = np.random.default_rng(31)
    xin = put(random_logits(rng, T, V, np.float64, scale=3.0))
    with dec.prefix_session([xin]) as s:
        at = [s.roots[0]]
        for _d in range(3):
            kids = s.extend([g.id for g in at for _c in range(1, V)], [c for _g in at for c in range(1, V)])
            for j, g in enumerate(at):
                nxt = next_array(g)
                for c, e in zip(range(1, V), kids[j * (V - 1):(j + 1) * (V - 1)]):
                    want = lse([e.logp_end] + next_array(e).tolist())
                    assert abs(nxt[c] - want) <= SCORE_TOL, (g.tokens, c, nxt[c], want)
            at = [kids[2]] if _d == 0 else [kids[2], kids[3]]  # ([3]; then the repeat [3, 3] and [3, 4])
    return at


def run_surface(dec=None):
    """What needs no input on the device: the stubs, the refusals of streams and BPE texts"""
    from pyctcdecode_amd import PrefixSession, SessionPrefix, parallel  # noqa: F401
    from pyctcdecode_amd.parallel import DevicePool

    x = random_logits(np.random.default_rng(1), 10, 29)
    pool = object.__new__(DevicePool)  # (no workers started: the refusal comes first)
    with pytest.raises(NotImplementedError):
        pool.prefix_session([x])
    with pytest.raises(NotImplementedError):
        parallel.prefix_session_sharded(dec, [x])
