"""Phrase spotting (spot / spot_batch) on the CPU simulator, which runs the body of ctc_spot (csrc/ctc_align.h) with a
one-thread context: the event by enumeration, the numpy recursion of tests/spot_util.py at the lengths where the kernels
change shape, a ragged batch, the edges and find's refusals. The HIP build: tests/test_gpu_spot.py, on the same checks."""
import itertools
import math

import numpy as np
import pytest

from tests.score_util import normalisation_input
from tests.sim_util import sim_library  # noqa: F401
from tests.spot_util import (HALF_MARGIN, check_spot, enumerate_occurrences, feasible, length_cases, lp_matrix, random_logits,
                             random_target, same, spot_np)
from tests.test_align import build

TINY = [(3, 6), (4, 5)]
LENGTHS = length_cases()
LENGTH_IDS = ["L%d_T%d" % c[:2] for c in LENGTHS]


def check_enumeration(V, T):
    """Every phrase of 1 to 3 labels, [a, a] and [a, b, a] among them: per end frame, and in the count, the summed weight of
    all V^T paths that have a maximal occurrence ending there."""
    x = normalisation_input(V, T)
    table = enumerate_occurrences(x, 0)
    phrases = [list(p) for n in (1, 2, 3) for p in itertools.product(range(1, V), repeat=n)]
    worst = worst_count = 0.0
    for p, g in zip(phrases, build(V).spot(x, tokens=phrases, trace=True)):
        want = table.get(tuple(p), np.zeros(T))
        worst = max(worst, float(np.max(np.abs(np.exp(g.end_logp) - want))))
        worst_count = max(worst_count, abs(g.count - float(want.sum())))
    print("V=%d T=%d: %d phrases, worst gap to the enumeration %.2e per frame, %.2e in the count" % (V, T, len(phrases), worst, worst_count))
    assert worst <= 1e-12 and worst_count <= 1e-12


def check_length_case(case, to_input=lambda x: x):
    L, T, phrase, x = case
    dec = build(29)
    got = dec.spot(to_input(x), tokens=[phrase], max_hits=3, trace=True)[0]
    assert dec.last_spot_launched == ((1, 0) if L <= 127 else (0, 1)) and dec.last_spot_launches == 1
    sure = check_spot(got, x, phrase, 0, max_hits=3, what="L=%d T=%d" % (L, T))
    assert np.array_equal(sure, np.isfinite(got.end_logp))
    plain = dec.spot(x, tokens=[phrase], max_hits=3)[0]
    assert plain.end_logp is None and plain.end_start is None and (plain.hits, plain.count) == (got.hits, got.count)


def check_ragged_batch(to_input=lambda x: x):
    """Utterances with 3, 0, 1, 3, 1 and 2 phrases, one too long for its utterance and one above the wave kernel's length:
    the batch equals the single calls, in one pair of launches and under a trace budget that forces three. -> xs, phrases, batch"""
    rng = np.random.default_rng(14)
    xs, phrases = [], []
    for T, count in ((40, 3), (25, 0), (61, 1), (9, 3), (300, 1), (33, 2)):
        xs.append(random_logits(rng, T, 29))
        phrases.append([random_target(rng, int(rng.integers(1, 9)), 29) for _ in range(count)])
    phrases[3][2] = random_target(rng, 12, 29)  # (12 labels, 9 frames)
    phrases[4][0] = random_target(rng, 130, 29, doubled=3)
    dec = build(29)
    ins = [to_input(x) for x in xs]
    batch = dec.spot_batch(ins, tokens=phrases, max_hits=3, trace=True)
    assert dec.last_spot_launched == (8, 1) and dec.last_spot_launches == 2 and [len(b) for b in batch] == [3, 0, 1, 3, 1, 2]
    for u, cur in enumerate(phrases):
        assert all(same(a, b) for a, b in zip(batch[u], dec.spot(ins[u], tokens=cur, max_hits=3, trace=True))), u
        for p, g in zip(cur, batch[u]):
            if feasible(len(xs[u]), p):
                check_spot(g, xs[u], p, 0, max_hits=3, what="utt %d" % u)
    split = dec.spot_batch(ins, tokens=phrases, max_hits=3, trace=True, _trace_budget=12 * 300)
    assert dec.last_spot_launches >= 3 and sum(dec.last_spot_launched) == 9
    assert all(same(a, b) for cur_a, cur_b in zip(batch, split) for a, b in zip(cur_a, cur_b))
    return xs, phrases, batch


@pytest.mark.parametrize("V,T", TINY)
def test_the_event_by_enumeration(V, T, sim_library):  # noqa: F811
    check_enumeration(V, T)


def test_the_chosen_seeds_leave_no_trace_entry_out():
    for L, T, phrase, x in LENGTHS:
        end_logp, mean, _ = spot_np(lp_matrix(x), phrase, 0)
        fin = np.isfinite(end_logp)
        assert fin.any() and np.all(np.abs(mean[fin] - np.floor(mean[fin]) - 0.5) > HALF_MARGIN), (L, T)


@pytest.mark.parametrize("case", LENGTHS, ids=LENGTH_IDS)
def test_against_numpy(case, sim_library):  # noqa: F811
    check_length_case(case)


def test_batch_equals_single_calls(sim_library):  # noqa: F811
    check_ragged_batch()


def test_edges(sim_library):  # noqa: F811
    dec = build(29)
    got = dec.spot(np.zeros((0, 29)), tokens=[[2, 3], [4]], max_hits=2, trace=True)
    assert [(g.hits, g.count, g.end_logp.shape) for g in got] == [([], 0.0, (0,))] * 2 and dec.last_spot_launches == 0
    assert dec.spot_batch([], []) == [] and dec.spot(np.zeros((4, 29)), []) == []
    rng = np.random.default_rng(3)
    got = dec.spot(random_logits(rng, 5, 29), tokens=[[9, 6, 13, 13, 16]], trace=True)[0]  # (six frames are needed)
    assert got.hits == [] and got.count == 0.0 and dec.last_spot_launched == (0, 0)
    assert np.all(got.end_logp == -np.inf) and np.all(got.end_start == -1) and got.end_logp.shape == (5,)
    # probabilities whose frame 3 is label 7 with probability exactly 1: fresh_4 and right_2 of [7] are -inf
    p = np.exp(lp_matrix(random_logits(rng, 12, 29)))
    p /= p.sum(axis=1, keepdims=True)
    p[3] = 0.0
    p[3, 7] = 1.0
    for phrase in ([7], [7, 9], [9, 7], [7, 7]):
        got = dec.spot(p, tokens=[phrase], max_hits=4, trace=True)[0]
        check_spot(got, p, phrase, 0, max_hits=4, what="p = 1, phrase %s" % phrase)
    assert got.end_logp[2] == -np.inf  # ([7, 7] cannot end on frame 2 either)
    one = dec.spot(p, tokens=[[7]], trace=True)[0]
    assert one.end_logp[2] == -np.inf and one.end_start[2] == -1 and np.isfinite(one.end_logp[3]) and one.end_start[4] <= 3
    # -inf logits on the phrase's labels: the emissions take the floor, every score stays finite
    x = random_logits(rng, 25, 29)
    phrase = random_target(rng, 5, 29, doubled=1)
    for t in range(0, 25, 3):
        x[t, phrase[(t // 3) % 5]] = -np.inf
    got = dec.spot(x, tokens=[phrase], max_hits=3, trace=True)[0]
    check_spot(got, x, phrase, 0, max_hits=3, what="-inf logits")
    assert got.hits and math.isfinite(got.count)
    assert dec.spot(x, tokens=[phrase], max_hits=3, min_logp=got.hits[0].logp)[0].hits == got.hits[:1]
    assert dec.spot(x, tokens=[phrase], min_logp=math.inf)[0].hits == []


def test_refusals_are_finds(sim_library, monkeypatch):  # noqa: F811
    from pyctcdecode_amd.decoder import _ResidentBeams
    from pyctcdecode_amd.parallel import DevicePool, spot_batch_sharded

    dec = build(5)
    x = np.zeros((9, 5))
    long_x, long_phrase = np.zeros((2100, 5)), random_target(np.random.default_rng(1), 2048, 5)
    refused = [(x, dict(texts="ab"), "utterance 0.*bare str"), (x, dict(tokens=[[2], [0]]), "utterance 0, phrase 1.*label id"),
               (x, dict(tokens=[[2], []]), "utterance 0, phrase 1 is empty"), (x, dict(texts=[[2, 3]]), "utterance 0, phrase 0 is not a str"),
               (x, dict(texts=["ab"], max_hits=65), "max_hits"), (x, dict(texts=["ab"], max_hits=True), "max_hits"),
               (x, dict(texts=["ab"], min_logp=float("nan")), "min_logp"), (x, dict(texts=["ab"], tokens=[[2, 3]]), "exactly one"),
               (x, dict(texts=["ab z"]), "'z'"), (long_x, dict(tokens=[long_phrase]), "utterance 0, phrase 0.*limit of 2047"),
               (np.zeros((9, 6)), dict(texts=["ab"]), None)]
    for logits, kwargs, match in refused:
        for call in (dec.spot, dec.find):  # (find's own refusal of the same call)
            with pytest.raises(ValueError, match=match):
                call(logits, **kwargs)
    with pytest.raises(ValueError, match="utterance 0, phrase 0.*budget"):
        dec.spot_batch([x], [["ab"]], _trace_budget=12 * 9 - 1)
    monkeypatch.setenv("CTCDEC_FIND_KERNEL", "warp")
    with pytest.raises(ValueError, match="CTCDEC_FIND_KERNEL"):
        dec.spot(x, ["ab"])
    monkeypatch.delenv("CTCDEC_FIND_KERNEL")
    with DevicePool(dec, devices=[0], library=sim_library.path) as pool:
        for call in (lambda: dec.spot(_ResidentBeams.__new__(_ResidentBeams), ["ab"]), lambda: pool.spot(x, ["a"]),
                     lambda: dec.spot_batch([_ResidentBeams.__new__(_ResidentBeams)], [["ab"]]),
                     lambda: spot_batch_sharded(dec, [x], [["a"]])):
            with pytest.raises(NotImplementedError):
                call()
    assert len(dec.spot(x, ["ab"])[0].hits) == 1  # (the decoder still works)
