"""Alignment with gaps (align_gaps / align_gaps_batch) on the CPU simulator of the kernels, which runs the bodies of
csrc/ctc_align.h themselves with a one-thread context: every shape case of tests/align_gaps_util.py under every gap pattern
against the numpy yardstick (the probability case and the float16 ties case among them), a gap-free target against align
exactly, planted inputs on which the frames themselves are known -- the tie rule among them --, batches against single calls
in one launch and in several, texts against tokens, the refusals of the Python surface and of the C entry point. The HIP
build: tests/test_gpu_align_gaps.py, which runs the bodies below on the device."""
import numpy as np
import pytest

from tests.align_gaps_util import (FOLDS, GAP, MAX_LABELS, PATTERNS, case_input, check_gapped, equals_plain, gap_cases,
                                   gaps_of_pattern, items_of, same_gapped)
from tests.align_util import feasible, random_logits, random_target
from tests.find_util import neg_inf_case, planted_input
from tests.sim_util import sim_library  # noqa: F401
from tests.test_align import build, ragged_batch

CASES = gap_cases()


def identity(x):
    return x


def run_shape_case(case, to_input=identity):
    """One shape case under every pattern it has a slot for. `to_input`: what the calls are given for the host array (the GPU
    tests pass a device tensor as well). Returns {pattern: result}."""
    name, V, T, target, _dtype, _kind = case
    dec = build(V)
    x = case_input(case)
    xin = to_input(x)
    L = len(target)
    tight = T == L + sum(1 for a, b in zip(target, target[1:]) if a == b)
    patterns = ("none", "both") if name == "limit_L2047" else PATTERNS
    folds = (None,) + (FOLDS if T <= 60 else ("mean",))
    plain = {fold: dec.align(xin, tokens=target, confidence=fold) for fold in folds}
    every = dec.align_gaps(xin, tokens=items_of(target, [1] * (L + 1))).score
    out = {}
    for pattern in patterns:
        gaps = gaps_of_pattern(pattern, target)
        if gaps is None:
            continue
        for fold in folds if pattern in ("none", "both") else ("mean",):
            a = dec.align_gaps(xin, tokens=items_of(target, gaps), confidence=fold)
            check_gapped(a, x, target, gaps, dec, fold, "%s %s %s" % (name, pattern, fold), plain[fold].score, every)
            if pattern == "none":  # the same path, frames, confidences and score as align: exactly
                assert equals_plain(a, plain[fold]), (name, fold)
            if tight:
                # no frame to spare: every gap is empty and the path holds no -1 -- but for a gap between two equal labels,
                # which by the definition takes the one frame the blank between them would
                slots = [j for j in range(L + 1) if gaps[j]]
                forced = [0 < j < L and target[j - 1] == target[j] for j in slots]
                assert [e - s for s, e in a.gaps] == [1 if f else 0 for f in forced], (name, pattern, a.gaps)
                assert all(f or v == 0.0 for f, v in zip(forced, a.gap_logp)), (name, pattern)
                assert int((a.path == GAP).sum()) == sum(forced), (name, pattern)
        out[pattern] = a
    if name == "T1_L1":
        assert out["both"].path.tolist() == target and out["both"].gaps == [(0, 0), (1, 1)]
    return out


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_shape_cases(case, sim_library):  # noqa: F811
    run_shape_case(case)


def test_the_cases_cover_what_they_should():
    names = [c[0] for c in CASES]
    for must in ("T1_L1", "T_eq_L_no_blanks", "hello_at_bound", "aaa_at_bound", "limit_L2047", "V29_probs", "V29_f16_ties",
                 "L511_T1100", "L512_T1100"):
        assert must in names
    assert all(len(c[3]) >= 1 for c in CASES)
    chunks = {c[0]: (2 * len(c[3]) + 1 + 3) // 4 for c in CASES}
    assert chunks["L511_T1100"] == 256 and chunks["L512_T1100"] == 257  # (256 threads up to 256 groups of states, 1024 above)
    for name in ("T_eq_L_no_blanks", "hello_at_bound", "aaa_at_bound"):
        c = CASES[names.index(name)]
        assert feasible(c[2], c[3]) and not feasible(c[2] - 1, c[3])
    assert any(gaps_of_pattern("doubled", c[3]) is not None for c in CASES)


# ---- planted inputs: the frames themselves are known (+30: a margin of nats, not rounding) ------------------------------
def run_planted_phrase(to_input=identity):
    V, T, blank = 29, 90, 0
    dec = build(V)
    rng = np.random.default_rng(101)
    phrase = random_target(rng, 6, V, doubled=1)
    x, windows = planted_input(rng, T, V, phrase, blank, [37])
    xin = to_input(x)
    gaps = [1] + [0] * (len(phrase) - 1) + [1]
    a = dec.align_gaps(xin, tokens=items_of(phrase, gaps), confidence="mean")
    check_gapped(a, x, phrase, gaps, dec, "mean", "planted phrase", dec.align(xin, tokens=phrase).score,
                 dec.align_gaps(xin, tokens=items_of(phrase, [1] * (len(phrase) + 1))).score)
    window = (a.token_frames[0][1][0], a.token_frames[-1][1][1])
    assert window == windows[0], (window, windows)
    hit = dec.find(xin, tokens=[phrase])[0].hits[0]
    assert (hit.start, hit.end) == window, (hit, window)
    assert a.gaps == [(0, window[0]), (window[1], T)]


def run_planted_pair(to_input=identity):
    V, blank, noise = 29, 0, 30
    dec = build(V)
    labels = dec._alphabet.labels
    rng = np.random.default_rng(102)
    w1, w2 = "bugs", "bunny"
    y1, y2 = [labels.index(c) for c in w1], [labels.index(c) for c in w2]
    s2 = 2 * len(y1) + noise
    T = s2 + 2 * len(y2) - 1  # (the matrix starts on the first word's first label and ends on the second word's last)
    x = rng.standard_normal((T + 1, V))
    for s0, y in ((0, y1), (s2, y2)):
        for k, c in enumerate(y):
            x[s0 + 2 * k, c] += 30.0
            x[s0 + 2 * k + 1, blank] += 30.0
    x = x[:T]
    win1, win2 = (0, 2 * len(y1) - 1), (s2, T)
    xin = to_input(x)
    a = dec.align_gaps(xin, "%s * %s" % (w1, w2), confidence="min")
    gaps = [0] * len(y1) + [1] + [0] * len(y2)
    plain = dec.align(xin, tokens=y1 + y2)
    check_gapped(a, x, y1 + y2, gaps, dec, "min", "planted pair", plain.score,
                 dec.align_gaps(xin, tokens=items_of(y1 + y2, [1] * (len(gaps)))).score)
    assert a.text == "%s * %s" % (w1, w2) and a.tokens == y1 + [GAP] + y2
    assert a.text_frames == [(w1, win1), (w2, win2)], (a.text_frames, win1, win2)
    assert a.gaps == [(win1[1], win2[0])], (a.gaps, win1, win2)
    print("planted pair: with the gap %.6f, align on the concatenated labels %.6f, difference %.6f"
          % (a.score, plain.score, a.score - plain.score))
    assert a.score - plain.score > 10.0, (a.score, plain.score)


def run_planted_ties(to_input=identity):
    """A label that is its row's maximum emits g(t), bit for bit: "the label keeps this frame" and "the gap already has it"
    tie exactly. With step preferred in the gap and stay in the label, every label keeps all three of its frames -- the first
    after the leading gap and the last before the trailing gap included."""
    V, T, blank = 29, 44, 0
    dec = build(V)
    rng = np.random.default_rng(5)
    target = [7, 12, 12, 5]
    x = rng.standard_normal((T, V))
    t, want = 10, []
    for c in target:
        x[t:t + 3, c] += 30.0
        want.append((t, t + 3))
        x[t + 3, blank] += 30.0
        t += 4
    xin = to_input(x)
    gaps = [1, 0, 0, 0, 1]
    a = dec.align_gaps(xin, tokens=items_of(target, gaps), confidence="mean")
    check_gapped(a, x, target, gaps, dec, "mean", "planted ties", dec.align(xin, tokens=target).score,
                 dec.align_gaps(xin, tokens=items_of(target, [1] * 5)).score)
    assert [f for _lab, f in a.token_frames] == want, (a.token_frames, want)
    assert a.gaps == [(0, want[0][0]), (want[-1][1], T)], a.gaps


def test_planted_phrase_is_found_where_it_lies(sim_library):  # noqa: F811
    run_planted_phrase()


def test_planted_pair_with_a_gap_between(sim_library):  # noqa: F811
    run_planted_pair()


def test_tie_rule_gives_a_label_all_of_its_frames(sim_library):  # noqa: F811
    run_planted_ties()


# ---- the rest ----------------------------------------------------------------------------------------------------------
def gapped_batch(seed=5, n=33):
    """ragged_batch of tests/test_align.py without its empty targets, each target under a pattern of its own."""
    xs, targets = ragged_batch(n=n, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    keep = [u for u, t in enumerate(targets) if t]
    xs, targets = [xs[u] for u in keep], [targets[u] for u in keep]
    all_gaps = []
    for u, t in enumerate(targets):
        gaps = gaps_of_pattern(PATTERNS[u % len(PATTERNS)], t)
        all_gaps.append(gaps if gaps is not None else rng.integers(0, 2, len(t) + 1).tolist())
    return xs, targets, all_gaps


def run_batch_equals_single_calls(to_input=identity):
    dec = build(29)
    xs, targets, all_gaps = gapped_batch()
    assert len(xs) >= 25
    xin = [to_input(x) for x in xs]
    items = [items_of(t, g) for t, g in zip(targets, all_gaps)]
    batch = dec.align_gaps_batch(xin, tokens=items, confidence="mean")
    assert dec.last_align_gaps_launches == 1 and len(dec.last_align_gaps_timing_ms) == 4
    for u, (x, target, gaps) in enumerate(zip(xs, targets, all_gaps)):
        check_gapped(batch[u], x, target, gaps, dec, "mean", "utt %d" % u)
        assert same_gapped(batch[u], dec.align_gaps(xin[u], tokens=items[u], confidence="mean")), u
    return dec, xs, xin, targets, all_gaps, items, batch


def run_tiny_budget(to_input=identity):
    dec = build(29)
    xs, targets, all_gaps = gapped_batch(seed=11)
    xin = [to_input(x) for x in xs]
    items = [items_of(t, g) for t, g in zip(targets, all_gaps)]
    whole = dec.align_gaps_batch(xin, tokens=items, confidence="max")
    assert dec.last_align_gaps_launches == 1
    biggest = max(len(x) * ((2 * len(t) + 1 + 3) // 4) for x, t in zip(xs, targets))
    split = dec.align_gaps_batch(xin, tokens=items, confidence="max", _bp_budget=biggest)
    assert dec.last_align_gaps_launches > 3
    assert all(same_gapped(a, b) for a, b in zip(whole, split))


def test_batch_equals_single_calls(sim_library):  # noqa: F811
    dec, xs, _xin, targets, _all_gaps, items, batch = run_batch_equals_single_calls()
    # the same utterances padded into one [B, T, V] array: every row of an utterance is a frame
    T = max(len(x) for x in xs)
    pad = np.zeros((len(xs), T, 29))
    for u, x in enumerate(xs):
        pad[u, : len(x)] = x
    cube = dec.align_gaps_batch(pad, tokens=items, confidence="mean")
    for u in range(len(xs)):
        assert same_gapped(cube[u], dec.align_gaps(pad[u], tokens=items[u], confidence="mean")), u


def test_tiny_budget_takes_several_launches(sim_library):  # noqa: F811
    run_tiny_budget()


def test_text_against_tokens(sim_library):  # noqa: F811
    dec = build(29)
    labels = dec._alphabet.labels
    ids = lambda s: [labels.index(c) for c in s]  # noqa: E731
    rng = np.random.default_rng(8)
    x = random_logits(rng, 60, 29)
    sp = labels.index(" ")
    for text, items, norm in (("* bugs bunny", [GAP] + ids("bugs") + [sp] + ids("bunny"), "* bugs bunny"),
                              ("  bugs *   bunny\n", ids("bugs") + [GAP] + ids("bunny"), "bugs * bunny"),
                              ("bugs * * bunny *", ids("bugs") + [GAP, GAP] + ids("bunny") + [GAP], "bugs * bunny *")):
        a = dec.align_gaps(x, text, confidence="min")
        b = dec.align_gaps(x, tokens=items, confidence="min")
        assert a.text == norm and same_gapped(a, b), (text, a.text, b.text)
        merged = [c for k, c in enumerate(items) if not (c == GAP and k and items[k - 1] == GAP)]
        assert a.tokens == merged and [w for w, _ in a.text_frames] == ["bugs", "bunny"]
        target = [c for c in merged if c != GAP]
        gaps = [0] * (len(target) + 1)
        k = 0
        for c in merged:
            if c == GAP:
                gaps[k] = 1
            else:
                k += 1
        check_gapped(a, x, target, gaps, dec, "min", text)
    # another marker
    a = dec.align_gaps(x, "<gap> bugs", gap="<gap>")
    assert a.text == "<gap> bugs" and a.tokens == [GAP] + ids("bugs")
    with pytest.raises(ValueError, match=r"'\*'"):  # (under another marker the star is a character like any other)
        dec.align_gaps(x, "* bugs", gap="<gap>")


def test_strict_false_returns_none_for_the_infeasible(sim_library):  # noqa: F811
    dec = build(29)
    labels = dec._alphabet.labels
    rng = np.random.default_rng(3)
    target = [labels.index(c) for c in "hello"]
    items = [GAP] + target + [GAP]
    ok, short = random_logits(rng, 6, 29), random_logits(rng, 5, 29)
    with pytest.raises(ValueError, match="no path"):
        dec.align_gaps(short, tokens=items)
    with pytest.raises(ValueError, match=r"\[1\]"):
        dec.align_gaps_batch([ok, short], tokens=[items, items])
    got = dec.align_gaps_batch([ok, short, ok], tokens=[items, items, items], strict=False, confidence="min")
    assert got[1] is None and same_gapped(got[0], got[2])
    check_gapped(got[0], ok, target, [1, 0, 0, 0, 0, 1], dec, "min", "at the bound")
    assert GAP not in got[0].path.tolist()
    assert dec.align_gaps_batch([short], tokens=[items], strict=False) == [None]
    assert dec.align_gaps_batch([], tokens=[]) == []


def test_neg_inf_logits_keep_every_score_finite(sim_library):  # noqa: F811
    dec = build(29)
    x, phrase = neg_inf_case()
    for pattern in PATTERNS:
        gaps = gaps_of_pattern(pattern, phrase)
        if gaps is None:
            continue
        a = dec.align_gaps(x, tokens=items_of(phrase, gaps), confidence="mean")
        assert np.isfinite(a.score) and np.all(np.isfinite(a.gap_logp)) and np.all(np.isfinite(a.token_logp)), pattern
        check_gapped(a, x, phrase, gaps, dec, "mean", "-inf %s" % pattern, dec.align(x, tokens=phrase).score)
    # a row without a number: its gap frame takes the floor, as every NaN entry does
    y = x.copy()
    y[7] = np.nan
    a = dec.align_gaps(y, tokens=[GAP] + phrase + [GAP])
    assert np.isfinite(a.score) and np.all(np.isfinite(a.gap_logp))


def test_python_refusals(sim_library):  # noqa: F811
    from pyctcdecode_amd import GappedAlignment, build_ctcdecoder

    dec = build(29)
    x = np.zeros((30, 29))
    assert isinstance(dec.align_gaps(x, "* ab"), GappedAlignment)
    for bad in ("", " ", "a b", "*\t"):
        with pytest.raises(ValueError, match="gap marker"):
            dec.align_gaps(x, "ab", gap=bad)
    with pytest.raises(ValueError, match="label of the alphabet"):
        dec.align_gaps(x, "a b c", gap="a")
    for text in ("", "*", " * * "):
        with pytest.raises(ValueError, match="utterance 0 has no label"):
            dec.align_gaps(x, text)
    with pytest.raises(ValueError, match="utterance 1 has no label"):
        dec.align_gaps_batch([x, x], tokens=[[2], [GAP]])
    rng = np.random.default_rng(1)
    long = random_target(rng, MAX_LABELS + 1, 29)
    with pytest.raises(ValueError, match="utterance 1 has 2048 target labels, above the limit of 2047"):
        dec.align_gaps_batch([x, np.zeros((2100, 29))], tokens=[[2], [GAP] + long])
    with pytest.raises(ValueError, match="1 targets for 2"):
        dec.align_gaps_batch([x, x], "ab")
    with pytest.raises(ValueError, match="1 targets for 1"):
        dec.align_gaps_batch([x], "ab")
    with pytest.raises(ValueError, match=r"texts\[1\] is not a str"):
        dec.align_gaps_batch([x, x], ["ab", ["a"]])
    for bad in ([0], [29], [-2], [2.0], [True]):
        with pytest.raises(ValueError, match=r"tokens\[0\] holds"):
            dec.align_gaps(x, tokens=bad)
    with pytest.raises(ValueError, match="exactly one"):
        dec.align_gaps(x, "ab", tokens=[2, 3])
    with pytest.raises(ValueError, match="exactly one"):
        dec.align_gaps_batch([x])
    with pytest.raises(ValueError, match="'!'"):
        dec.align_gaps(x, "ab * !")
    with pytest.raises(ValueError):
        dec.align_gaps(x, "ab", confidence="median")
    with pytest.raises(ValueError, match="budget"):
        dec.align_gaps_batch([np.zeros((400, 29))], tokens=[[GAP] + long[:100]], _bp_budget=1000)
    bpe = build_ctcdecoder(["<unk>", "▁bug", "s", "▁bun", "ny", "▁", "n", "▁a"])
    assert bpe._alphabet.is_bpe
    xb = np.zeros((12, len(bpe._alphabet.labels)))
    with pytest.raises(ValueError, match="tokens="):
        bpe.align_gaps(xb, "bugs * bunny")
    lab = bpe._alphabet.labels
    a = bpe.align_gaps(xb, tokens=[lab.index("▁bug"), lab.index("s"), GAP, lab.index("▁bun"), lab.index("ny")])
    assert a.text == "bugs * bunny" and [w for w, _ in a.text_frames] == ["bugs", "bunny"]


def test_parallel_refuses(sim_library):  # noqa: F811
    from pyctcdecode_amd.parallel import DevicePool, align_gaps_batch_sharded

    dec = build(5)
    with pytest.raises(NotImplementedError):
        align_gaps_batch_sharded(dec, [np.zeros((3, 5))], ["a *"])
    with DevicePool(dec, devices=[0], library=sim_library.path) as pool:
        with pytest.raises(NotImplementedError):
            pool.align_gaps_batch([np.zeros((3, 5))], ["a *"])
        with pytest.raises(NotImplementedError):
            pool.align_gaps(np.zeros((3, 5)), "a *")


def test_native_call_validates_what_it_indexes_with(sim_library):  # noqa: F811
    """The C entry point on its own: adjacent gaps, a target without a label, the blank, a label outside the alphabet, an
    infeasible pair, too many labels (gaps do not count) and a table above the budget are error codes before anything is
    launched; the gaps of an alignment made without them are refused."""
    import ctypes as C

    dec = build(5)
    dll = dec._lib.dll
    blank = dec._alphabet.labels.index("")
    x = np.zeros((4200, 5))

    def call(target, frames=4, off=None, budget=0, plain=False):
        ptrs = (C.c_void_p * 1)(x.ctypes.data)
        fr = (C.c_int32 * 1)(frames)
        t = np.array(target or [0], dtype=np.int32)
        o = np.array(off or [0, len(target)], dtype=np.int64)
        res = C.c_void_p()
        fn = dll.ctcdec_align_batch if plain else dll.ctcdec_align_gaps_batch
        rc = fn(dec._handle, ptrs, fr, 1, 1, 0, t.ctypes.data_as(C.POINTER(C.c_int32)), o.ctypes.data_as(C.POINTER(C.c_int64)), 0,
                budget, C.byref(res))
        if rc != 0:
            return rc, None
        go, gs, ge, gl, ng = (C.POINTER(C.c_int64)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_double)(),
                              C.c_int64())
        grc = dll.ctcdec_alignment_gaps(res, C.byref(go), C.byref(gs), C.byref(ge), C.byref(gl), C.byref(ng))
        n = int(ng.value) if grc == 0 else None
        dll.ctcdec_alignment_free(res)
        return grc, n

    assert call([2, 3]) == (0, 0) and call([-1, 2, -1, 3, -1]) == (0, 3)
    assert call([2, 3], plain=True) == (-1, None)  # (ctcdec_alignment_gaps on a plain alignment)
    assert call([2, -1, -1, 3])[0] == -1
    assert call([-1])[0] == -1 and call([])[0] == -1
    assert call([2, blank])[0] == -1 and call([2, 5])[0] == -1 and call([-2, 2])[0] == -1
    assert call([2, -1, 2, 2])[0] == -1  # (needs five frames: a gap between equal labels does not lift the bound)
    assert call([2, -1, 2], frames=3) == (0, 1)  # (the gap between equal labels takes the frame a blank would)
    assert call([2, 3], off=[0, -1])[0] == -1 and call([2, 3], off=[1, 2])[0] == -1
    assert call([2, 3], frames=-1)[0] == -1
    many = [2, 3] * 1024
    assert call([-1] + many[:MAX_LABELS] + [-1], frames=4200)[0] == 0  # (2047 labels and two gaps)
    assert call(many[:MAX_LABELS + 1], frames=4200)[0] == -4
    assert call([2, 3, -1] * 20, frames=400, budget=1000)[0] == -4
