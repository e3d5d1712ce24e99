"""The transcript calls at the batch sizes their benchmarks run at (tests/test_gpu_transcript_scale.py on the HIP build,
tests/test_transcript_scale.py on the simulator): the inputs, the harness, and the list of places where results are checked.

Part 1, the wide batch: N utterances that are small in every dimension but the count, with utterances without frames, targets
without an alignment and five 300-frame utterances whose targets straddle the wave kernel's 127 labels planted at fixed
places (planted()). One call over all N is compared, bit for bit, with the same utterances handed over in reverse order in
calls of 7 (whole_against_small), with itself under each alternate route, at sample_places() with the numpy yardstick of the
call's own util at that util's tolerance, and at the planted places with what the small-batch tests assert there. Nothing here
introduces a tolerance: every bound is SCORE_TOL / GAMMA_TOL / GRAD_TOL of the utils, every equality is `==` on the floats.

Part 2, tables of 2 to 4 GiB and the default budgets: the counts are computed from the decoder's own table formulas and budget
constants (posteriors_plan, align_plan, launches_under); the CPU twin asserts them without allocating anything.

Part 3, more than 65535 prefix rows that nothing is launched for (dead_rows_case)."""
import numpy as np

from pyctcdecode_amd import decoder as D
from tests import align_long_util, find_util, grad_util, posteriors_util, prefix_util, score_util
from tests.align_gaps_util import PATTERNS, check_gapped, gaps_of_pattern, items_of, same_gapped
from tests.align_util import char_labels, check_aligned, feasible, random_target
from tests.greedy_util import check_greedy, of_batch, same_batch_entry
from tests.test_find import same as same_found
from tests.test_score import check_score

BLANK = 0          # of tests/align_util.char_labels
N_BENCH = 4096     # the utterances tools/align_bench.py and the README's figures run
N_GPU = N_BENCH + 37  # no multiple of 4, 16, 64 or 256; more one-workgroup-per-utterance launches than 256 CUs hold at once
N_SIM = 301
CHUNK = 7          # utterances of a small call
N_PLACES = 64      # places that go against numpy
LONG_T = 300
LONG_LABELS = (127, 128, 129, 127, 129)  # the wave kernel's last length and the group kernel's first two
WAVE_MAX_LABELS = score_util.WAVE_MAX_LABELS
DENSE_SLICE = 256  # utterances of the dense posteriors call
# name -> (V, dtype, largest T of an ordinary utterance)
PARAMS = {"V29_f64": (29, np.float64, 48), "V1024_f16": (1024, np.float16, 24), "V131_f16": (131, np.float16, 24)}


def planted(n):
    """-> (no frames, no alignment, 300 frames): the fixed places of an n-utterance batch"""
    t0 = [0, 5, 64, 129, n // 3, n // 2, 3 * n // 4, n - 1]
    bad = [2, 63, 128, 200, n // 3 + 7, n // 2 + 9, 3 * n // 4 + 5, n - 3]
    long = [7, 90, n // 2 + 3, n - 40, n - 5]
    every = t0 + bad + long
    assert len(set(every)) == len(every) and min(every) == 0 and max(every) == n - 1, n
    return t0, bad, long


def sample_places(n, seed=64):
    """The N_PLACES utterances that go against numpy: the first and the last, the indices either side of every multiple of
    256 below 1025, the neighbours of every planted utterance without frames or without an alignment, the 300-frame
    utterances, and the rest from a seeded generator."""
    t0, bad, long = planted(n)
    want = [0, n - 1]
    for m in range(256, 1025, 256):
        want += [m - 1, m, m + 1]
    for p in t0 + bad:
        want += [p - 1, p + 1]
    want += long
    places = []
    for p in want:
        if 0 <= p < n and p not in places:
            places.append(p)
    assert len(places) <= N_PLACES, len(places)
    rest = [int(u) for u in np.random.default_rng(seed).permutation(n) if int(u) not in places]
    places += rest[: N_PLACES - len(places)]
    assert len(places) == N_PLACES == len(set(places))
    return places


class Batch:
    """One wide batch: xs[u] the host matrix of utterance u (a view of one array), targets[u] its transcript, gap_items[u] /
    gap_targets[u] / gap_flags[u] the target of align_gaps (at least one label; gaps in about half), items[u] the 0 to 3
    hypotheses / prefixes of score and prefix_scores, phrases[u] the same number of non-empty phrases of find."""

    def __init__(self, n, V, dtype, max_t, seed=2025):
        rng = np.random.default_rng(seed + V)
        self.n, self.V, self.dtype = n, V, np.dtype(dtype)
        self.t0, self.bad, self.long = planted(n)
        frames = rng.integers(1, max_t + 1, size=n)
        frames[self.t0] = 0
        frames[self.bad] = [3 + k % 2 for k in range(len(self.bad))]
        frames[self.long] = LONG_T
        self.frames = [int(t) for t in frames]
        self.targets, self.items, self.phrases = [], [], []
        self.gap_targets, self.gap_flags, self.gap_items = [], [], []
        long_labels = dict(zip(self.long, LONG_LABELS))
        for u, T in enumerate(self.frames):
            if u in long_labels:
                target = random_target(rng, long_labels[u], V, doubled=4)
            elif u in self.bad:
                # (3 frames: five labels; 4 frames: four labels and a repeat, one frame below the bound)
                target = random_target(rng, 5, V) if T == 3 else random_target(rng, 4, V, doubled=1)
            else:
                L = int(rng.integers(0, min(T, 12) + 1))
                doubled = min(int(rng.integers(0, 3)), max(0, L - 1), T - L)
                target = random_target(rng, L, V, doubled=doubled) if L else []
            self.targets.append(target)
            one = random_target(rng, 1, V)
            gt = target if target else one
            flags = gaps_of_pattern(PATTERNS[int(rng.integers(1, len(PATTERNS)))], gt) if u % 2 == 0 else None
            flags = flags if flags is not None else [0] * (len(gt) + 1)
            self.gap_targets.append(gt)
            self.gap_flags.append(flags)
            self.gap_items.append(items_of(gt, flags))
            # 1 to 3 items, none for one utterance in fifty; a planted utterance always has its target and one label more
            pool = [list(target), list(target[: len(target) // 2]), list(target) + random_target(rng, 2, V),
                    random_target(rng, int(rng.integers(1, 5)), V)]
            count = 0 if u % 50 == 10 else int(rng.integers(1, 4))
            if u in self.t0 + self.bad + self.long:
                count = 2
                pool = [list(target), one]
            self.items.append(pool[:count])
            self.phrases.append([list(p) if p else random_target(rng, int(rng.integers(1, 4)), V) for p in pool[:count]])
        if sum(len(cur) for cur in self.items) % 2 == 0:  # (an odd number of items: the last wave of a launch is partial)
            self.items[1].append(random_target(rng, 2, V))
            self.phrases[1].append(random_target(rng, 2, V))
        self.n_items = sum(len(cur) for cur in self.items)
        assert self.n_items % 2 == 1 and any(not cur for cur in self.items)
        row0 = np.zeros(n + 1, dtype=np.int64)
        row0[1:] = np.cumsum(self.frames)
        self.row0 = row0
        wide = self.dtype == np.float64
        self.data = (rng.standard_normal((int(row0[-1]), V), dtype=np.float64 if wide else np.float32) * 3.0).astype(self.dtype)
        self.xs = [self.data[row0[u]:row0[u + 1]] for u in range(n)]
        for u in self.bad:
            assert not feasible(self.frames[u], self.targets[u])

    def ref(self, u):
        """Utterance u as the numpy yardsticks take it: the exact values, float64 as they are, float16 widened to float32"""
        return self.xs[u] if self.dtype == np.float64 else self.xs[u].astype(np.float32)

    def on_device(self):
        """Every utterance as a view of one device tensor"""
        import torch

        dev = torch.from_numpy(self.data).cuda()
        return [dev[self.row0[u]:self.row0[u + 1]] for u in range(self.n)]

    def launched(self, items, forced_group=False):
        """(wave, group): the items of `items[u]` a forward or find kernel is launched for, by kernel"""
        live = [p for u, cur in enumerate(items) for p in cur if self.frames[u] > 0 and feasible(self.frames[u], p)]
        wave = 0 if forced_group else sum(1 for p in live if len(p) <= WAVE_MAX_LABELS)
        return wave, len(live) - wave


_BATCHES = {}


def batch_of(name, n):
    """The batch of a parametrisation, made once and never changed"""
    if (name, n) not in _BATCHES:
        V, dtype, max_t = PARAMS[name]
        _BATCHES[name, n] = Batch(n, V, dtype, max_t)
    return _BATCHES[name, n]


def build(V):
    from pyctcdecode_amd import build_ctcdecoder

    return build_ctcdecoder(char_labels(V))


# ---- the harness ---------------------------------------------------------------------------------------------------------------
def or_none(same):
    """A comparison of two results, either of which may be the None of an utterance without an alignment"""
    return lambda a, b: (a is b) if a is None or b is None else bool(same(a, b))


def each(same):
    """A comparison of two utterances' lists of results"""
    return lambda a, b: len(a) == len(b) and all(same(p, q) for p, q in zip(a, b))


def whole_against_small(run, same, n, what):
    """`run(idx)` -> the results of utterances idx, in that order. The one call over all n equals, place for place, the same
    utterances in reverse order in calls of CHUNK. Returns the whole call's results."""
    whole = run(list(range(n)))
    assert len(whole) == n, (what, len(whole))
    rev = list(range(n))[::-1]
    differ, seen = [], 0
    for k in range(0, n, CHUNK):
        idx = rev[k:k + CHUNK]
        part = run(idx)
        assert len(part) == len(idx), (what, k)
        for u, got in zip(idx, part):
            seen += 1
            if not same(whole[u], got):
                differ.append(u)
    assert seen == n
    assert not differ, "%s: %d of %d places of the whole call differ from their small call, first %s" % (
        what, len(differ), n, differ[:8])
    return whole


def equal_everywhere(whole, other, same, what):
    differ = [u for u in range(len(whole)) if not same(whole[u], other[u])]
    assert len(whole) == len(other) and not differ, "%s: %d places differ, first %s" % (what, len(differ), differ[:8])


def sub(seq, idx):
    return [seq[u] for u in idx]


class Scale:
    """The checks of one batch on one library build. `xin`: the utterances as the large call takes them; `host`: the same as host
    arrays when xin are device tensors (the alternate route of part 1b), else None; `monkeypatch`: pytest's, for the kernel
    switches."""

    def __init__(self, b, xin, monkeypatch, host=None):
        self.b, self.xin, self.host, self.mp = b, xin, host, monkeypatch
        self.dec = build(b.V)
        self.places = sample_places(b.n)
        self.device = host is not None

    # -- score --------------------------------------------------------------------------------------------------------------------
    def score(self):
        b, dec = self.b, self.dec
        run = lambda idx, xin=self.xin: dec.score_batch(sub(xin, idx), tokens=sub(b.items, idx))  # noqa: E731
        same = each(lambda p, q: p == q)
        self.mp.delenv("CTCDEC_FORWARD_KERNEL", raising=False)
        whole = whole_against_small(run, same, b.n, "score")
        whole = run(list(range(b.n)))
        assert dec.last_score_launched == b.launched(b.items) and min(dec.last_score_launched) > 0, dec.last_score_launched
        for kernel in ("wave", "group"):
            self.mp.setenv("CTCDEC_FORWARD_KERNEL", kernel)
            forced = run(list(range(b.n)))
            assert dec.last_score_launched == b.launched(b.items, kernel == "group"), (kernel, dec.last_score_launched)
            equal_everywhere(whole, forced, same, "score under the %s kernel" % kernel)
        self.mp.delenv("CTCDEC_FORWARD_KERNEL")
        if self.host is not None:
            equal_everywhere(whole, run(list(range(b.n)), self.host), same, "score from host arrays")
        assert sum(len(cur) for cur in whole) == b.n_items
        for u in self.places + b.t0 + b.bad:
            for j, (p, got) in enumerate(zip(b.items[u], whole[u])):
                assert got.tokens == p
                check_score(got.logp, score_util.yardstick(b.ref(u), p, BLANK), "score utt %d item %d" % (u, j))
        for u in b.t0 + b.bad:
            want = [(0.0 if not p else -np.inf) if b.frames[u] == 0 else (-np.inf if not feasible(b.frames[u], p) else None)
                    for p in b.items[u]]
            assert -np.inf in want
            for w, got in zip(want, whole[u]):
                assert (np.isfinite(got.logp) if w is None else got.logp == w), (u, got.logp, w)
        return whole

    # -- align, align_long, align_gaps -----------------------------------------------------------------------------------------
    def _aligned(self, what, call, same, targets, check):
        b = self.b
        run = lambda idx, xin=self.xin: call(sub(xin, idx), sub(targets, idx))  # noqa: E731
        same = or_none(same)
        whole = whole_against_small(run, same, b.n, what)
        if self.host is not None:
            equal_everywhere(whole, run(list(range(b.n)), self.host), same, what + " from host arrays")
        for u in self.places:
            if whole[u] is None:
                assert not feasible(b.frames[u], [c for c in targets[u] if c >= 0]), (what, u)
            else:
                check(whole[u], u)
        for u in b.bad:
            assert whole[u] is None, (what, u)
        return whole

    def align(self):
        b, dec = self.b, self.dec
        check = lambda a, u: check_aligned(a, b.ref(u), b.targets[u], dec, None, "align utt %d" % u)  # noqa: E731
        whole = self._aligned("align", lambda xs, t: dec.align_batch(xs, tokens=t, strict=False), align_long_util.same, b.targets,
                              check)
        for u in b.t0:  # (no frames, no labels: the one empty alignment)
            a = whole[u]
            assert a.text == "" and a.score == 0.0 and a.path.shape == (0,) and a.token_frames == [] and a.text_frames == [], u
        return whole

    def align_long(self):
        b, dec = self.b, self.dec
        check = lambda a, u: check_aligned(a, b.ref(u), b.targets[u], dec, None, "align_long utt %d" % u)  # noqa: E731
        whole = self._aligned("align_long", lambda xs, t: dec.align_long_batch(xs, tokens=t, strict=False), align_long_util.same,
                              b.targets, check)
        keep = [u for u in range(b.n) if whole[u] is not None]
        # (the plan a call reports is the last call's: the whole batch once more)
        equal_everywhere(whole, dec.align_long_batch(self.xin, tokens=b.targets, strict=False), or_none(align_long_util.same),
                         "align_long a second time")
        assert dec.last_align_long_plan == [align_long_util.plan_of(b.frames[u], 0) for u in keep]
        cut = self._aligned("align_long in segments of 7 frames",
                            lambda xs, t: dec.align_long_batch(xs, tokens=t, strict=False, _segment_frames=7), align_long_util.same,
                            b.targets, check)
        equal_everywhere(cut, dec.align_long_batch(self.xin, tokens=b.targets, strict=False, _segment_frames=7),
                         or_none(align_long_util.same), "align_long in segments a second time")
        assert dec.last_align_long_plan == [align_long_util.plan_of(b.frames[u], 7) for u in keep]
        assert max(n_seg for _k, n_seg in dec.last_align_long_plan) == -(-(LONG_T - 1) // 7)
        equal_everywhere(whole, cut, or_none(align_long_util.same), "align_long whole against segments")
        plain = dec.align_batch(self.xin, tokens=b.targets, strict=False)
        equal_everywhere(whole, plain, or_none(align_long_util.same), "align_long against align")
        for u in b.t0:
            assert whole[u].text == "" and whole[u].score == 0.0 and whole[u].path.shape == (0,), u
        return whole

    def align_gaps(self):
        b, dec = self.b, self.dec
        assert sum(1 for f in b.gap_flags if any(f)) >= b.n // 3

        def check(a, u):
            # (the two bounds check_gapped holds a score between, from calls of the utterance alone as in tests/test_align_gaps.py)
            t = b.gap_targets[u]
            plain = dec.align(self.xin[u], tokens=t).score
            every = dec.align_gaps(self.xin[u], tokens=items_of(t, [1] * (len(t) + 1))).score
            check_gapped(a, b.ref(u), t, b.gap_flags[u], dec, None, "align_gaps utt %d" % u, plain_score=plain,
                         every_score=every)

        whole = self._aligned("align_gaps", lambda xs, t: dec.align_gaps_batch(xs, tokens=t, strict=False), same_gapped,
                              b.gap_items, check)
        for u in b.t0:  # (a target of align_gaps has a label: without frames it has no path)
            assert whole[u] is None, u
        return whole

    # -- posteriors, gradient ------------------------------------------------------------------------------------------------------
    def posteriors(self):
        b, dec = self.b, self.dec
        lean_same = or_none(lambda p, q: posteriors_util.same_bits(p, q, dense=False))

        def run(idx, xin=self.xin):
            return dec.posteriors_batch(sub(xin, idx), tokens=sub(b.targets, idx), dense=False, strict=False)

        whole = whole_against_small(run, lean_same, b.n, "posteriors")
        whole = run(list(range(b.n)))
        n_live = sum(1 for u in range(b.n) if b.frames[u] > 0 and whole[u] is not None)
        assert dec.last_posteriors_launched == (n_live, 0) and dec.last_posteriors_launches == 1, dec.last_posteriors_launched
        if self.host is not None:
            equal_everywhere(whole, run(list(range(b.n)), self.host), lean_same, "posteriors from host arrays")
        # the dense call over a slice that holds planted utterances of every kind, and the large call's summaries against it
        lo = max(0, b.n // 2 - DENSE_SLICE // 2 + 12)
        sl = list(range(lo, min(b.n, lo + DENSE_SLICE)))
        assert {b.t0[5], b.bad[5], b.long[2]} <= set(sl)

        def dense_run(idx):
            utts = [sl[k] for k in idx]
            return dec.posteriors_batch(sub(self.xin, utts), tokens=sub(b.targets, utts), strict=False)

        dense = whole_against_small(dense_run, or_none(posteriors_util.same_bits), len(sl), "dense posteriors")
        for k, u in enumerate(sl):
            assert lean_same(whole[u], dense[k]), u
        for u in self.places + b.t0:
            got, t = whole[u], b.targets[u]
            if got is None:
                assert not feasible(b.frames[u], t), u
                continue
            assert got.gamma is None and got.token_post is None
            want = posteriors_util.yardstick(b.ref(u), t, BLANK)
            # the table of this utterance from a call of its own: the large call's summaries are its bits, and it goes
            # through every check of the util
            alone = dense[sl.index(u)] if u in sl else dec.posteriors(self.xin[u], tokens=t)
            assert posteriors_util.same_bits(got, alone, dense=False), u
            posteriors_util.check_posteriors(alone, want, b.frames[u], t, "posteriors utt %d" % u)
        for u in b.t0:
            assert whole[u].logp == 0.0 and whole[u].logp_backward == 0.0 and whole[u].occupancy.shape == (0,), u
        for u in b.bad:
            assert whole[u] is None, u
        return whole

    def gradient(self):
        b, dec = self.b, self.dec
        same = or_none(grad_util.same_bits)
        run = lambda idx, xin=self.xin: dec.gradient_batch(sub(xin, idx), tokens=sub(b.targets, idx), strict=False)  # noqa: E731
        whole = whole_against_small(run, same, b.n, "gradient")
        whole = run(list(range(b.n)))
        assert dec.last_gradient_launches == 2 and dec.last_gradient_launched[1] == 0, dec.last_gradient_launches
        if self.device:
            import torch

            # every utterance's rows are a view of the call's one device allocation, in input order
            at = base = whole[0].grad.untyped_storage().data_ptr()
            for u in range(b.n):
                if whole[u] is None:
                    continue
                g = whole[u].grad
                assert isinstance(g, torch.Tensor) and g.device == self.xin[0].device and g.untyped_storage().data_ptr() == base, u
                assert tuple(g.shape) == (b.frames[u], b.V) and (g.data_ptr() == at or b.frames[u] == 0), u
                at += b.frames[u] * b.V * g.element_size()
            equal_everywhere(whole, run(list(range(b.n)), self.host), same, "gradient from host arrays")
        for u in self.places + b.t0:
            got, t = whole[u], b.targets[u]
            if got is None:
                assert not feasible(b.frames[u], t), u
                continue
            x = b.ref(u)
            grad = grad_util.check_gradient(got, grad_util.grad_np(x, t, BLANK), x, t, "gradient utt %d" % u, on_device=self.device)
            if b.frames[u]:
                grad_util.check_rows(grad, x, t, BLANK, "gradient utt %d" % u)
        for u in b.t0:
            assert whole[u].logp == 0.0 and tuple(whole[u].grad.shape) == (0, b.V), u
        for u in b.bad:
            assert whole[u] is None, u
        return whole

    # -- find ---------------------------------------------------------------------------------------------------------------------
    def find(self):
        b, dec = self.b, self.dec

        def run(idx, xin=self.xin):
            return dec.find_batch(sub(xin, idx), tokens=sub(b.phrases, idx), max_hits=3, trace=True)

        same = each(same_found)
        self.mp.delenv("CTCDEC_FIND_KERNEL", raising=False)
        whole = whole_against_small(run, same, b.n, "find")
        whole = run(list(range(b.n)))
        assert dec.last_find_launched == b.launched(b.phrases) and min(dec.last_find_launched) > 0, dec.last_find_launched
        for kernel in ("wave", "group"):
            self.mp.setenv("CTCDEC_FIND_KERNEL", kernel)
            forced = run(list(range(b.n)))
            assert dec.last_find_launched == b.launched(b.phrases, kernel == "group"), (kernel, dec.last_find_launched)
            equal_everywhere(whole, forced, same, "find under the %s kernel" % kernel)
        self.mp.delenv("CTCDEC_FIND_KERNEL")
        if self.host is not None:
            equal_everywhere(whole, run(list(range(b.n)), self.host), same, "find from host arrays")
        for u in self.places + b.t0 + b.bad:
            for j, (p, got) in enumerate(zip(b.phrases[u], whole[u])):
                find_util.check_found(got, b.ref(u), p, BLANK, max_hits=3, what="find utt %d phrase %d" % (u, j))
        for u in b.t0 + b.bad:
            for p, got in zip(b.phrases[u], whole[u]):
                if not feasible(b.frames[u], p):
                    assert got.hits == [] and got.end_logp.shape == (b.frames[u],) and np.all(got.end_logp == -np.inf) and \
                        np.all(got.end_start == -1), u
            assert any(not feasible(b.frames[u], p) for p in b.phrases[u]), u
        return whole

    # -- greedy -------------------------------------------------------------------------------------------------------------------
    def greedy(self):
        b, dec = self.b, self.dec
        run = lambda idx, xin=self.xin: dec.decode_greedy_batch(sub(xin, idx))  # noqa: E731
        texts = whole_against_small(run, lambda p, q: p == q, b.n, "decode_greedy")

        def run_conf(idx, xin=self.xin):
            t, frames = dec.decode_greedy_batch(sub(xin, idx), token_frames=True, confidence="mean")
            assert len(frames) == len(idx)
            return [of_batch(t, frames, k, dec) for k in range(len(idx))]

        conf = whole_against_small(run_conf, lambda p, q: p == q, b.n, "decode_greedy with confidences")
        assert [c[0] for c in conf] == texts
        if self.host is not None:
            assert run(list(range(b.n)), self.host) == texts
            equal_everywhere(conf, run_conf(list(range(b.n)), self.host), lambda p, q: p == q, "decode_greedy from host arrays")
        for u in self.places + b.t0:
            g = dec.decode_greedy(self.xin[u], confidence="mean")
            assert same_batch_entry(conf[u], g), u
            check_greedy(g, b.ref(u), dec, "mean", "greedy utt %d" % u)
        for u in b.t0:
            assert texts[u] == "" and conf[u] == ("", [], [], 0.0), (u, conf[u])
        return texts, conf

    # -- prefix scores ------------------------------------------------------------------------------------------------------------
    def prefix_scores(self):
        b, dec = self.b, self.dec
        run = lambda idx, xin=self.xin: dec.prefix_scores_batch(sub(xin, idx), tokens=sub(b.items, idx))  # noqa: E731
        same = each(prefix_util.same_prefix)
        self.mp.delenv("CTCDEC_FORWARD_KERNEL", raising=False)
        whole = whole_against_small(run, same, b.n, "prefix_scores")
        whole = run(list(range(b.n)))
        assert dec.last_prefix_launched == b.launched(b.items) and min(dec.last_prefix_launched) > 0, dec.last_prefix_launched
        if self.device:
            self.one_block(dec.last_prefix_next, [g for cur in whole for g in cur], b.n_items)
        for kernel in ("wave", "group"):
            self.mp.setenv("CTCDEC_FORWARD_KERNEL", kernel)
            forced = run(list(range(b.n)))
            assert dec.last_prefix_launched == b.launched(b.items, kernel == "group"), (kernel, dec.last_prefix_launched)
            equal_everywhere(whole, forced, same, "prefix_scores under the %s kernel" % kernel)
        self.mp.delenv("CTCDEC_FORWARD_KERNEL")
        if self.host is not None:
            equal_everywhere(whole, run(list(range(b.n)), self.host), same, "prefix_scores from host arrays")
        for u in self.places + b.t0 + b.bad:
            for j, (p, got) in enumerate(zip(b.items[u], whole[u])):
                prefix_util.check_prefix(got, b.ref(u), p, BLANK, "prefix_scores utt %d prefix %d" % (u, j))
        for u in b.t0 + b.bad:
            dead = 0
            for p, got in zip(b.items[u], whole[u]):
                if b.frames[u] == 0 or not feasible(b.frames[u], p):
                    dead += 1
                    assert got.logp_end == (0.0 if b.frames[u] == 0 and not p else -np.inf), (u, p, got.logp_end)
                    assert np.isneginf(prefix_util.next_array(got)).all(), (u, p)
            assert dead, u
        return whole

    def one_block(self, block, results, count):
        """The ownership of a device call's results: every next_logp is row h of the call's one [count, V] tensor"""
        import torch

        assert isinstance(block, torch.Tensor) and block.is_cuda and block.dtype == torch.float64
        assert tuple(block.shape) == (count, self.b.V), tuple(block.shape)
        assert len(results) == count
        base, first, step = block.untyped_storage().data_ptr(), block.data_ptr(), block.stride(0) * block.element_size()
        for h, g in enumerate(results):
            assert g.next_logp.untyped_storage().data_ptr() == base and g.next_logp.data_ptr() == first + h * step, h
            assert tuple(g.next_logp.shape) == (self.b.V,), h

    # -- prefix session -----------------------------------------------------------------------------------------------------------
    def walk_session(self, xin, on_device):
        """A session over all n utterances: three children per root, a third of them extended again -- half of those by their
        own last label --, half of the 4 n slots released and extended into. The arena holds exactly the 5 n prefixes that are
        live at the fullest, so the last extension can only go into released slots. Returns every prefix formed, released
        ones included: roots, children, grandchildren, late children."""
        dec, n, V = self.dec, self.b.n, self.b.V
        rng = np.random.default_rng(n)
        with dec.prefix_session(xin, capacity=5 * n) as s:
            roots = s.roots
            assert [r.utt for r in roots] == list(range(n))
            steps = [(roots, s.last_next)]
            kids = s.extend([r.id for r in roots for _ in range(3)], [int(c) for c in rng.integers(1, V, size=3 * n)])
            assert s.last_launches[0] == 1 and s.last_launches[2:] == (0, 0), s.last_launches
            steps.append((kids, s.last_next))
            third = kids[::3]
            labels = [k.tokens[-1] if j % 2 == 0 else int(rng.integers(1, V)) for j, k in enumerate(third)]
            grand = s.extend([k.id for k in third], labels)
            steps.append((grand, s.last_next))
            assert len(s) == 5 * n == s.capacity
            gone = (kids + grand)[::2]
            s.release([g.id for g in gone])
            assert len(s) == 3 * n
            left = (kids + grand)[1::2]
            parents = [left[j % len(left)] if j % 4 else roots[j % n] for j in range(2 * n)]
            late = s.extend([p.id for p in parents], [int(c) for c in rng.integers(1, V, size=2 * n)])
            steps.append((late, s.last_next))
            assert len(s) == 5 * n and s.last_launches[0] == 1 and s.last_launches[2:] == (0, 0), s.last_launches
            for node, p in zip(late, parents):
                assert node.utt == p.utt and node.tokens[:-1] == p.tokens
            if on_device:
                for step, block in steps:
                    self.one_block(block, step, len(step))
        return roots + kids + grand + late

    def prefix_session(self):
        """Every prefix of walk_session's session equals prefix_scores_batch of its labels, asked a few hundred prefixes at a
        time; the session over host arrays gives the same bits."""
        b, dec = self.b, self.dec
        nodes = self.walk_session(self.xin, self.device)
        assert len(nodes) == 7 * b.n
        differ = []
        for k in range(0, len(nodes), 301):
            part = nodes[k:k + 301]
            utts = sorted({g.utt for g in part})
            at = {u: j for j, u in enumerate(utts)}
            per_utt = [[] for _ in utts]
            for g in part:
                per_utt[at[g.utt]].append(g)
            got = dec.prefix_scores_batch(sub(self.xin, utts), tokens=[[g.tokens for g in cur] for cur in per_utt])
            for cur, res in zip(per_utt, got):
                assert len(cur) == len(res)
                differ += [(g.utt, g.tokens) for g, w in zip(cur, res) if not prefix_util.same_prefix(g, w)]
        assert not differ, "%d of %d session prefixes differ from prefix_scores_batch, first %s" % (
            len(differ), len(nodes), differ[:4])
        if self.host is not None:
            from_host = self.walk_session(self.host, False)
            assert [(g.utt, g.tokens) for g in from_host] == [(g.utt, g.tokens) for g in nodes]
            equal_everywhere(nodes, from_host, prefix_util.same_prefix, "session over host arrays")
        by_utt = {}
        for g in nodes:
            by_utt.setdefault(g.utt, []).append(g)
        for k, u in enumerate(self.places):
            mine = by_utt[u]
            for g in ([mine[0]] if k < 8 else []) + [mine[-1]]:  # (the empty prefix at eight places; the last prefix formed)
                prefix_util.check_prefix(g, b.ref(u), g.tokens, BLANK, "session utt %d %s" % (u, g.tokens))
        for u in b.t0:
            for g in by_utt[u]:
                assert g.logp_end == (0.0 if not g.tokens else -np.inf), (u, g.tokens, g.logp_end)
                assert np.isneginf(prefix_util.next_array(g)).all(), (u, g.tokens)
        return nodes


ENTRY_POINTS = ("score", "align", "align_gaps", "align_long", "posteriors", "gradient", "find", "greedy", "prefix_scores",
                "prefix_session")


# ---- part 2: the plans of the large tables --------------------------------------------------------------------------------
TABLE_T, TABLE_L, TABLE_V = 512, 255, 29  # 511 states, 128 groups of four: 2 MiB of tables per utterance
BP_T, BP_L = 2048, 1023                   # 512 groups, a byte per frame and group: 1 MiB of back-pointers per utterance
TABLE_UTTS_ONE_LAUNCH, TABLE_UTTS_SPLIT, BP_UTTS = 1100, 2200, 1100
SMALL_LAUNCH_UTTS = 16
TABLE_INPUTS = 8


def launches_under(sizes, budget):
    """How many launches a call makes of utterances with tables of `sizes` bytes, in order, under a budget: a launch takes
    utterances while the sum stays within the budget (budget_groups, csrc/api_transcript.cpp)"""
    launches, held = 0, 0
    for s in sizes:
        assert s <= budget
        if s == 0:  # (no frames: no table, in no launch)
            continue
        if launches == 0 or held + s > budget:
            launches, held = launches + 1, 0
        held += s
    return launches


def posteriors_plan(n):
    """-> (bytes per utterance, bytes of the call, launches under the default budget, the budget that admits SMALL_LAUNCH_UTTS a
    launch, launches under it)"""
    per = D.BeamSearchDecoderCTC._state_table_bytes(TABLE_T, TABLE_L)
    small = SMALL_LAUNCH_UTTS * per
    return per, n * per, launches_under([per] * n, D.POSTERIORS_TABLE_BUDGET), small, launches_under([per] * n, small)


def align_plan(n):
    """-> (bytes per utterance, bytes of the call, launches under the default budget, the budget of one utterance a launch)"""
    per = D.BeamSearchDecoderCTC._bp_table_bytes(BP_T, BP_L)
    return per, n * per, launches_under([per] * n, D.ALIGN_BP_BUDGET), per


def around_mark(per, n, mark_bytes):
    """The first utterance, the last, and those either side of `mark_bytes` of cumulative table bytes"""
    mark = mark_bytes // per  # (the utterance whose table starts at the mark, or holds it)
    assert 1 <= mark < n - 2, (per, n)
    return [0, mark - 1, mark, mark + 1, n - 1]


def table_targets(n, L, V=TABLE_V, seed=512):
    rng = np.random.default_rng(seed)
    return [random_target(rng, L, V, doubled=4) for _ in range(n)]


# ---- part 3: prefix rows that nothing is launched for ------------------------------------------------------------------------
FILL_PIECE = 65535  # rows of one ctc_prefix_fill launch (PrefixExtend::stage, csrc/api_transcript.cpp)
DEAD_FRAMES = (0, 6, 1)
DEAD_SHARE = (1000, 20000)  # dead rows of the first two utterances: the piece boundary falls among the third's


def dead_rows_case(n_dead=FILL_PIECE + 3, n_live=300, V=29, seed=3):
    """-> (xs, prefixes[u], dead[u][j]): three utterances of 0, 6 and 1 frames and n_dead prefixes that nothing is launched
    for, interleaved with n_live live ones. dead[u][j] is the position of prefix j of utterance u in the call's list of
    dead rows -- the rows follow the utterances --, -1 for a live one. A live prefix goes before every dead row from position
    65530 on and after the last, so that the rows 65534 to 65537 each have a live row on either side; the others are spread
    evenly over the two utterances that have frames."""
    rng = np.random.default_rng(seed)
    xs = [(rng.standard_normal((T, V)) * 3.0) for T in DEAD_FRAMES]
    # (without frames even the empty prefix is a row nothing is launched for; the others are too long for 6 frames and for 1)
    dead_of = ([[], [2], [3, 4]], [[2, 2, 3, 3, 4, 4], [5, 6, 7, 8, 9, 10, 11]], [[2, 3], [4, 4]])
    live_of = (None, [[], [2], [3, 3], [4, 5, 6], [7, 8, 8, 9]], [[], [5]])
    share = list(DEAD_SHARE) + [n_dead - sum(DEAD_SHARE)]
    assert share[2] > 0 and sum(share[:2]) < FILL_PIECE - 8 < n_dead
    before = set(range(FILL_PIECE - 5, n_dead))
    before |= set(np.linspace(share[0], FILL_PIECE - 6, n_live - len(before) - 1).astype(int).tolist())
    prefixes, dead = [[], [], []], [[], [], []]
    d = 0
    for u in range(3):
        k_live = 0
        for k in range(share[u]):
            if d in before and live_of[u]:
                prefixes[u].append(list(live_of[u][k_live % len(live_of[u])]))
                dead[u].append(-1)
                k_live += 1
            prefixes[u].append(list(dead_of[u][k % len(dead_of[u])]))
            dead[u].append(d)
            d += 1
    prefixes[2].append([5])  # (the live row after the last dead one)
    dead[2].append(-1)
    assert d == n_dead and [k for ks in dead for k in ks if k >= 0] == list(range(n_dead))
    for u, cur in enumerate(prefixes):
        for p, k in zip(cur, dead[u]):
            assert (k >= 0) == (DEAD_FRAMES[u] == 0 or not feasible(DEAD_FRAMES[u], p)), (u, p, k)
    return xs, prefixes, dead


def check_dead_rows(dec, xin, prefixes, dead, fills):
    """The call with the dead rows among the live ones: every dead row -inf in all columns, every live row the bits of the call
    with the live prefixes alone. `fills`: the ctc_prefix_fill launches the call must add to those of the call with the live
    prefixes alone (None: a build that counts no launches). Returns the flat [rows, V] next_logp on the host."""
    V = len(dec._alphabet.labels)
    live_only = [[p for p, k in zip(cur, ks) if k < 0] for cur, ks in zip(prefixes, dead)]
    alone = dec.prefix_scores_batch(xin, tokens=live_only)
    base = dec.last_prefix_launches
    got = dec.prefix_scores_batch(xin, tokens=prefixes)
    if fills is not None:
        assert dec.last_prefix_launches == (base[0], base[1], base[2] + fills), (dec.last_prefix_launches, base, fills)
    block = dec.last_prefix_next
    if block is not None:
        assert tuple(block.shape) == (sum(len(cur) for cur in prefixes), V)
        rows = block.cpu().numpy()
    else:
        rows = np.stack([prefix_util.next_array(g) for cur in got for g in cur])
    flat = np.array([k for ks in dead for k in ks])
    n_dead = int((flat >= 0).sum())
    assert n_dead > FILL_PIECE
    bad = np.flatnonzero(~np.isneginf(rows[flat >= 0]).all(axis=1))
    assert len(bad) == 0, "%d dead rows hold something else than -inf, first at positions %s of the dead list" % (len(bad), bad[:8])
    differ = []
    for u, (cur, ks) in enumerate(zip(got, dead)):
        j = 0
        for g, k in zip(cur, ks):
            if k >= 0:
                assert g.logp_end == (0.0 if DEAD_FRAMES[u] == 0 and not g.tokens else -np.inf), (u, k, g.logp_end)
                assert np.isneginf(prefix_util.next_array(g)).all() if k in range(FILL_PIECE - 1, FILL_PIECE + 3) else True
                continue
            if not prefix_util.same_prefix(g, alone[u][j]):
                differ.append((u, j))
            j += 1
        assert j == len(alone[u])
    assert not differ, "%d live rows differ from the call with the live prefixes alone, first %s" % (len(differ), differ[:8])
    # the rows 65534 to 65537 of the dead list sit between live rows, and those are finite where a label can follow
    for k in range(FILL_PIECE - 1, FILL_PIECE + 3):
        at = int(np.flatnonzero(flat == k)[0])
        assert flat[at - 1] == -1 and flat[at + 1] == -1, k
        for r in (at - 1, at + 1):
            assert not np.isnan(rows[r]).any() and rows[r][BLANK] == -np.inf, (k, r)
    return rows
