"""Tiled forced alignment of long transcripts (align_long(tiled=True); DESIGN.md "Forced alignment of long transcripts, tiled"),
shared by the CPU and GPU tests: the tile shapes every shape case is cut at and the comparisons with align and align_long."""
from tests.align_long_util import ABOVE, FOLDS, above_input, mixed_batch, same
from tests.align_util import check_aligned

# (_tile_groups, _tile_frames, _segment_blocks): the library's own, then shapes that put a state-block edge, a time-block edge
# and a segment edge inside 12-frame cases
CUTS = [(0, 0, 0), (1, 1, 1), (3, 5, 2), (2, 7, 1), (256, 64, 7)]
ABOVE_CUT = (100, 97, 2)


def cuts_of(name):
    return [(0, 0, 0), ABOVE_CUT] if name == "limit_L2047" else CUTS


def tiled(dec, xs, targets, cut=(0, 0, 0), **kw):
    return dec.align_long_batch(xs, tokens=targets, tiled=True, _tile_groups=cut[0], _tile_frames=cut[1], _segment_blocks=cut[2], **kw)


def check_plan(dec, shapes, cut):
    """What the call reports for utterances of (T, L): the Python rule's plan, and launches and tiles where there are frames"""
    plans = [dec._align_tiled_plan(T, L, 1 << 30, *cut) for T, L in shapes]
    assert dec.last_align_tiled_plan == [p[:6] for p in plans], (cut, dec.last_align_tiled_plan)
    assert dec.last_align_long_plan == [p[6:] for p in plans], (cut, dec.last_align_long_plan)
    live = any(T > 0 for T, _L in shapes)
    assert (dec.last_align_tiled_launches > 0) == live and dec.last_align_tiled_tiles >= dec.last_align_tiled_launches
    assert dec.last_align_tiled_groups == dec.last_align_long_launches == (1 if live else 0)


def check_equals_align(dec, x, target, name, inputs=None):
    """tiled == align at every tile shape and fold, from every form of x"""
    for fold in (None,) + FOLDS:
        want = dec.align(x, tokens=target, confidence=fold)
        for cut in cuts_of(name):
            for xin in inputs if inputs is not None else [x]:
                got = tiled(dec, [xin], [target], cut, confidence=fold)[0]
                assert same(got, want), (name, fold, cut)
                check_plan(dec, [(len(x), len(target))], cut)


def check_above(dec, case, inputs=None):
    """One case above 2047 labels: against numpy (check_aligned) and == align_long untiled, at the default plan and ABOVE_CUT.
    Returns the gap to numpy's optimum."""
    name = case[0]
    target, x = above_input(case)
    want = dec.align_long_batch([x], tokens=[target])[0]
    for xin in inputs if inputs is not None else [x]:
        for cut in ((0, 0, 0), ABOVE_CUT):
            assert same(tiled(dec, [xin], [target], cut)[0], want), (name, cut)
            check_plan(dec, [(len(x), len(target))], cut)
    gap = abs(want.score - check_aligned(want, x, target, dec, None, name))
    print("%s: |score - numpy optimum| = %.3e" % (name, gap))
    return gap


def check_mixed_batch(dec, xs_in):
    """mixed_batch() equal per utterance to align_long_batch untiled, the infeasible utterance None; also under a budget that
    splits it into several launch groups, and refused one byte under the largest utterance's plan"""
    xs, targets, bad = mixed_batch()
    want = dec.align_long_batch(xs, tokens=targets, confidence="mean", strict=False)
    got = tiled(dec, xs_in, targets, confidence="mean", strict=False)
    shapes = [(len(x), len(t)) for u, (x, t) in enumerate(zip(xs, targets)) if u != bad]
    check_plan(dec, shapes, (0, 0, 0))
    assert got[bad] is None and all(same(a, b) for u, (a, b) in enumerate(zip(got, want)) if u != bad)
    most = max(dec._align_tiled_plan(T, L, 1 << 30, 0, 0, 0)[5] for T, L in shapes)
    split = tiled(dec, xs_in, targets, confidence="mean", strict=False, _bp_budget=most)
    assert dec.last_align_tiled_groups > 1 and dec.last_align_long_launches == dec.last_align_tiled_groups
    assert all(same(a, b) for u, (a, b) in enumerate(zip(split, want)) if u != bad)
    return most


__all__ = ["ABOVE", "ABOVE_CUT", "CUTS", "check_above", "check_equals_align", "check_mixed_batch", "check_plan", "tiled"]
