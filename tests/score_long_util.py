"""Transcript likelihood of long transcripts (BeamSearchDecoderCTC.score_long / score_long_batch; DESIGN.md "Transcript
likelihood of long transcripts"), shared by the CPU and GPU tests: the tile shapes every shape case of tests/align_util.py is
cut at, the comparison with score -- equal with ==, bit for bit --, the cases above score's 2047 labels against the numpy
recursion of tests/score_util.py, and the batch of several hypotheses per utterance."""
import numpy as np

from tests.align_long_util import ABOVE, LONG_MAX_LABELS, SHAPES, above_input, build, case_input
from tests.align_util import feasible, random_logits, random_target
from tests.score_util import yardstick

ABOVE_TILE = (100, 97)  # (_tile_groups, _tile_frames) the cases above 2047 labels run at, next to the library's own plan


def tile_shapes(name, T):
    """(_tile_groups, _tile_frames) of a shape case: the library's choice, one, two and three groups to a state block -- a block
    boundary between any two groups --, by one frame, two, a length that divides nothing, one frame short of all, all, more
    than all. limit_L2047 takes five, to stay within seconds."""
    if name == "limit_L2047":
        return [(0, 0), (0, 7), (1, T), (3, 1000), ABOVE_TILE]
    return [(g, f) for g in (0, 1, 2, 3) for f in sorted({0, 1, 2, 7, T + 5} | {k for k in (T - 1, T) if k >= 1})]


def check_equals_score(dec, x, target, name, T, inputs=None):
    """score_long == score at every tile shape, with the plan the Python rule gives. `inputs`: the forms of x to score (host
    array, device tensor); every form must give the same bits. Returns whether the window kept tiles from being launched."""
    want = dec.score(x, tokens=[target])[0].logp
    launched, skipped = T > 0 and feasible(T, target), False
    for g, f in tile_shapes(name, T):
        for xin in inputs if inputs is not None else [x]:
            got = dec.score_long_batch([xin], tokens=[[target]], _tile_groups=g, _tile_frames=f)[0][0].logp
            assert got == want, (name, g, f, got, want)
            plan = dec._score_long_plan(T, len(target), 1 << 30, g, f)
            assert dec.last_score_long_plan == ([plan] if launched else []), (name, g, f, dec.last_score_long_plan)
            skipped |= launched and dec.last_score_long_tiles < plan[2] * plan[3]
    return skipped


def check_above(dec, case, inputs=None):
    """One case above 2047 labels: the library's plan and ABOVE_TILE equal to each other with ==, and within 8 T eps |want| of
    the numpy recursion -- a frame adds at most about eight roundings, each relative eps on values no larger than the score.
    Returns the gap."""
    name, _V, L, T, _doubled, _dtype = case
    target, x = above_input(case)
    got = []
    for xin in inputs if inputs is not None else [x]:
        for g, f in ((0, 0), ABOVE_TILE):
            got.append(dec.score_long_batch([xin], tokens=[[target]], _tile_groups=g, _tile_frames=f)[0][0].logp)
            assert dec.last_score_long_plan == [dec._score_long_plan(T, L, 1 << 30, g, f)], (name, g, f)
    assert all(v == got[0] for v in got), (name, got)
    want = yardstick(x, target, dec._alphabet.labels.index(""))
    gap, bound = abs(got[0] - want), 8 * T * np.finfo(np.float64).eps * abs(want)
    print("%s: |logp - numpy| = %.3e (bound %.3e, logp %.6f)" % (name, gap, bound, want))
    assert gap <= bound, (name, gap, bound)
    return gap


def hypotheses_batch(dtype=np.float64):
    """(xs, hyps, (utterance, hypothesis) without an alignment): two utterances over 29 labels with several hypotheses each --
    one above 2047 labels, 129 labels, 9, one longer than its utterance has frames, the empty one."""
    rng = np.random.default_rng(41)
    V = 29
    xs = [random_logits(rng, 2500, V).astype(dtype), random_logits(rng, 37, V).astype(dtype)]
    hyps = [[random_target(rng, 2100, V, doubled=3), random_target(rng, 129, V, doubled=4), random_target(rng, 2600, V), []],
            [random_target(rng, 9, V, doubled=1), [], random_target(rng, 40, V)]]
    return xs, hyps, ((0, 2), (1, 2))


def check_hypotheses_batch(dec, xs, hyps, dead, hosts=None):
    """The batch at the library's plan == at ABOVE_TILE == every hypothesis in a call of its own == the staged host copy ==
    score_batch where that call accepts the hypothesis; -inf exactly where there is no alignment."""
    batch = dec.score_long_batch(xs, tokens=hyps)
    assert dec.last_score_long_groups == 1 and len(dec.last_score_long_plan) == sum(map(len, hyps)) - len(dead)
    tiled = dec.score_long_batch(xs, tokens=hyps, _tile_groups=ABOVE_TILE[0], _tile_frames=ABOVE_TILE[1])
    for u, cur in enumerate(hyps):
        for k, ids in enumerate(cur):
            lp = batch[u][k].logp
            assert (lp == -np.inf) == ((u, k) in dead) and tiled[u][k].logp == lp, (u, k)
            assert dec.score_long(xs[u], tokens=[ids])[0].logp == lp, (u, k)
            if hosts is not None:
                assert dec.score_long(hosts[u], tokens=[ids])[0].logp == lp, (u, k)
            if len(ids) <= 2047:
                assert dec.score(xs[u], tokens=[ids])[0].logp == lp, (u, k)
    return batch


__all__ = ["ABOVE", "ABOVE_TILE", "LONG_MAX_LABELS", "SHAPES", "above_input", "build", "case_input", "check_above",
           "check_equals_score", "check_hypotheses_batch", "hypotheses_batch", "tile_shapes"]
