"""Forced alignment (align / align_batch) on the CPU simulator of the kernels, which runs the bodies of csrc/ctc_align.h
themselves with a one-thread context: every shape case of tests/align_util.py against the numpy Viterbi, the feasibility
bound and the limits, ragged batches through a list and a [B, T, V] array, a batch forced over a tiny back-pointer budget
into several launches, a BPE alphabet through tokens=, the refusals, and committed reference goldens whose top text is
aligned back to its logits. The HIP build: tests/test_gpu_align.py."""
import numpy as np
import pytest

from tests.align_util import (FOLDS, MAX_LABELS, case_input, char_labels, check_aligned, feasible, random_logits, random_target,
                              shape_cases, viterbi_np)
from tests.golden_util import load_cases
from tests.sim_util import sim_library  # noqa: F401
from tests.token_logp_util import lp_matrix

SHAPES = shape_cases()
GOLDEN, GOLDEN_IN = load_cases()
# reference goldens over character alphabets whose top text aligns, under the numpy yardstick alone, inside the reference's own
# word windows (test_golden_words_overlap_under_numpy holds that against the yardstick before anything of ours is asked)
GOLDEN_NAMES = ["toy_lm_default", "toy_nolm_16beams", "toy_trailing_space_lm", "libri_char", "rand_libri_flat_lm_1",
                "rand_libri_int_lm_5", "words_libri_lm", "words_libri_trigram_boost4"]


def build(V):
    from pyctcdecode_amd import build_ctcdecoder

    return build_ctcdecoder(char_labels(V))


def ragged_batch(n=33, V=29, seed=5, dtype=np.float64):
    rng = np.random.default_rng(seed)
    xs, targets = [], []
    for u in range(n):
        L = int(rng.integers(0, 24))
        target = random_target(rng, L, V, doubled=min(2, max(0, L - 1))) if L else []
        need = L + sum(1 for a, b in zip(target, target[1:]) if a == b)
        T = need + int(rng.integers(0, 40)) if u % 5 else need  # (every fifth utterance sits exactly at the bound)
        xs.append(random_logits(rng, max(T, 1 if L else 0), V, dtype))
        targets.append(target)
    return xs, targets


def same(a, b):
    return (a.text == b.text and np.array_equal(a.path, b.path) and a.score == b.score and a.token_frames == b.token_frames
            and a.text_frames == b.text_frames and a.token_logp == b.token_logp and a.word_logp == b.word_logp)


@pytest.mark.parametrize("case", SHAPES, ids=[c[0] for c in SHAPES])
def test_shape_cases(case, sim_library):  # noqa: F811
    name, V, T, target, _dtype, _kind = case
    dec = build(V)
    x = case_input(case)
    for fold in (None,) + (FOLDS if T <= 300 else ("mean",)):
        a = dec.align(x, tokens=target, confidence=fold)
        check_aligned(a, x, target, dec, fold, "%s %s" % (name, fold))


def test_one_frame_below_the_bound(sim_library):  # noqa: F811
    dec = build(29)
    labels = dec._alphabet.labels
    rng = np.random.default_rng(3)
    for text, T in (("hello", 6), ("aaa", 5)):
        target = [labels.index(c) for c in text]
        assert feasible(T, target) and not feasible(T - 1, target)
        ok, short = random_logits(rng, T, 29), random_logits(rng, T - 1, 29)
        check_aligned(dec.align(ok, text), ok, target, dec, None, text)
        with pytest.raises(ValueError, match="no path"):
            dec.align(short, text)
        with pytest.raises(ValueError, match=r"\[1\]"):
            dec.align_batch([ok, short], [text, text])
        got = dec.align_batch([ok, short, ok], [text, text, text], strict=False, confidence="min")
        assert got[1] is None
        check_aligned(got[0], ok, target, dec, "min", text)
        assert same(got[0], got[2])
    # no frames at all: only the empty target has a path (the empty one)
    empty = np.zeros((0, 29))
    a = dec.align(empty, "")
    assert a.text == "" and a.path.shape == (0,) and a.score == 0.0 and a.token_frames == [] and a.text_frames == []
    assert dec.align_batch([empty], ["a"], strict=False) == [None]


def test_limit_is_refused(sim_library):  # noqa: F811
    dec = build(5)
    rng = np.random.default_rng(1)
    target = random_target(rng, MAX_LABELS + 1, 5)
    with pytest.raises(ValueError, match="limit of 2047"):
        dec.align(np.zeros((2100, 5)), tokens=target)
    with pytest.raises(ValueError, match="budget"):
        dec.align_batch([np.zeros((400, 5))], tokens=[target[:100]], _bp_budget=1000)


def test_texts_words_and_spaces(sim_library):  # noqa: F811
    dec = build(29)
    labels = dec._alphabet.labels
    rng = np.random.default_rng(8)
    x = random_logits(rng, 40, 29)
    text = "  bugs   bunny \n"
    target = [labels.index(c) for c in "bugs bunny"]
    for fold in FOLDS:
        a = dec.align(x, text, confidence=fold)
        assert a.text == "bugs bunny" and [w for w, _ in a.text_frames] == ["bugs", "bunny"]
        assert [lab for lab, _ in a.token_frames] == list("bugsbunny")  # (the space label is no token)
        check_aligned(a, x, target, dec, fold, fold)


def test_ragged_batch_equals_single_calls(sim_library):  # noqa: F811
    dec = build(29)
    xs, targets = ragged_batch()
    assert len(xs) == 33
    batch = dec.align_batch(xs, tokens=targets, confidence="mean")
    for u, (x, target) in enumerate(zip(xs, targets)):
        check_aligned(batch[u], x, target, dec, "mean", "utt %d" % u)
        assert same(batch[u], dec.align(x, tokens=target, confidence="mean")), u
    # the same utterances padded into one [B, T, V] array: every row of an utterance is a frame, so the targets are aligned
    # to the padded length -- equal to the per-utterance calls on the padded matrices
    T = max(len(x) for x in xs)
    pad = np.zeros((len(xs), T, 29))
    for u, x in enumerate(xs):
        pad[u, : len(x)] = x
    cube = dec.align_batch(pad, tokens=targets, confidence="mean")
    for u, target in enumerate(targets):
        check_aligned(cube[u], pad[u], target, dec, "mean", "padded %d" % u)
        assert same(cube[u], dec.align(pad[u], tokens=target, confidence="mean")), u


def test_tiny_budget_takes_several_launches(sim_library):  # noqa: F811
    dec = build(29)
    xs, targets = ragged_batch(seed=11)
    whole = dec.align_batch(xs, tokens=targets, confidence="max")
    assert dec.last_align_launches == 1
    biggest = max(len(x) * ((2 * len(t) + 1 + 3) // 4) for x, t in zip(xs, targets))
    split = dec.align_batch(xs, tokens=targets, confidence="max", _bp_budget=biggest)
    assert dec.last_align_launches > 3
    assert all(same(a, b) for a, b in zip(whole, split))


def test_bpe_alphabet_through_tokens(sim_library):  # noqa: F811
    from pyctcdecode_amd import build_ctcdecoder

    pieces = ["<unk>", "▁bug", "s", "▁bun", "ny", "▁", "n", "▁a"]
    dec = build_ctcdecoder(pieces)
    labels = dec._alphabet.labels
    assert dec._alphabet.is_bpe
    target = [labels.index(p) for p in ("▁bug", "s", "▁bun", "n", "n", "ny", "▁a")]
    rng = np.random.default_rng(4)
    x = random_logits(rng, 25, len(labels))
    a = dec.align(x, tokens=target, confidence="mean")
    assert a.text == "bugs bunnnny a" and [w for w, _ in a.text_frames] == ["bugs", "bunnnny", "a"]
    check_aligned(a, x, target, dec, "mean", "bpe")
    with pytest.raises(ValueError, match="tokens="):
        dec.align(x, "bugs bunny")


def test_bad_arguments(sim_library):  # noqa: F811
    dec = build(5)
    labels = dec._alphabet.labels
    x = np.zeros((9, 5))
    with pytest.raises(ValueError, match="'z'"):
        dec.align(x, "ab z")
    for bad in ([labels.index("")], [5], [-1], [2.0], [True]):
        with pytest.raises(ValueError, match="label id"):
            dec.align(x, tokens=bad)
    with pytest.raises(ValueError, match="exactly one"):
        dec.align(x, "ab", tokens=[2, 3])
    with pytest.raises(ValueError, match="exactly one"):
        dec.align_batch([x])
    with pytest.raises(ValueError, match="2 targets for 1"):
        dec.align_batch([x], ["a", "b"])
    with pytest.raises(ValueError):
        dec.align(x, "ab", confidence="median")
    with pytest.raises(ValueError):
        dec.align(np.zeros((9, 6)), "ab")
    assert dec.align_batch([], []) == []


def test_native_call_validates_what_it_indexes_with(sim_library):  # noqa: F811
    """The C entry point on its own: a label outside the alphabet, the blank, a decreasing offset, an infeasible pair and
    too many labels are error codes before anything is launched."""
    import ctypes as C

    dec = build(5)
    blank = dec._alphabet.labels.index("")
    x = np.zeros((4, 5))

    def call(target, frames=4, off=None):
        ptrs = (C.c_void_p * 1)(x.ctypes.data)
        fr = (C.c_int32 * 1)(frames)
        t = np.array(target or [0], dtype=np.int32)
        o = np.array(off or [0, len(target)], dtype=np.int64)
        res = C.c_void_p()
        rc = dec._lib.dll.ctcdec_align_batch(dec._handle, ptrs, fr, 1, 1, 0, t.ctypes.data_as(C.POINTER(C.c_int32)),
                                             o.ctypes.data_as(C.POINTER(C.c_int64)), 0, 0, C.byref(res))
        if rc == 0:
            dec._lib.dll.ctcdec_alignment_free(res)
        return rc

    assert call([2, 3]) == 0
    assert call([2, 5]) == -1 and call([-1]) == -1 and call([blank]) == -1
    assert call([2, 2, 2]) == -1  # (needs five frames)
    assert call([2, 3], off=[0, -1]) == -1 and call([2, 3], off=[1, 2]) == -1
    assert call([2, 3], frames=-1) == -1
    assert call([2] * (MAX_LABELS + 1), frames=4) == -4


def test_parallel_refuses(sim_library):  # noqa: F811
    from pyctcdecode_amd.parallel import DevicePool, align_batch_sharded

    dec = build(5)
    with pytest.raises(NotImplementedError):
        align_batch_sharded(dec, [np.zeros((3, 5))], ["a"])
    with DevicePool(dec, devices=[0], library=sim_library.path) as pool:
        with pytest.raises(NotImplementedError):
            pool.align_batch([np.zeros((3, 5))], ["a"])


def golden_case(name):
    case = next(c for c in GOLDEN if c["name"] == name)
    x = GOLDEN_IN[case["input"]]
    top = case["expected"][0]
    return case, x, top["text"], [(w, s, e) for w, s, e in top["frames"]]


def overlaps(got, want):
    assert [w for w, _ in got] == [w for w, _, _ in want], (got, want)
    return all(s < we and ws < e for (_w, (s, e)), (_v, ws, we) in zip(got, want))


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_golden_words_overlap_under_numpy(name):
    """The yardstick alone: the numpy path of the reference's top text puts every word inside the reference's window."""
    from pyctcdecode_amd.alphabet import Alphabet
    from tests.align_util import spans_of

    case, x, text, frames = golden_case(name)
    labels = Alphabet.build_alphabet(case["labels"]).labels
    blank, space = labels.index(""), labels.index(" ")
    target = [labels.index(c) for c in " ".join(text.split())]
    _best, path = viterbi_np(lp_matrix(x), target, blank)
    words, cur = [], []
    for c, s, e in spans_of(path, blank):
        if c == space:
            words.append(cur)
            cur = []
        else:
            cur.append((labels[c], s, e))
    words.append(cur)
    got = [("".join(p for p, _, _ in w), (w[0][1], w[-1][2])) for w in words if w]
    assert overlaps(got, frames), (got, frames)


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_golden_words_overlap(name, sim_library):  # noqa: F811
    from pyctcdecode_amd import build_ctcdecoder

    assert len(GOLDEN_NAMES) >= 5
    case, x, text, frames = golden_case(name)
    dec = build_ctcdecoder(case["labels"])
    a = dec.align(x, text, confidence="mean")
    labels = dec._alphabet.labels
    check_aligned(a, x, [labels.index(c) for c in " ".join(text.split())], dec, "mean", name)
    assert overlaps(a.text_frames, frames), (a.text_frames, frames)
