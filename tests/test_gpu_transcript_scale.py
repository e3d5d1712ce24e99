"""GPU (-m gpu): the transcript calls -- score, align, align_gaps, align_long, posteriors, gradient, find, decode_greedy,
prefix_scores, prefix_session -- at the batch sizes their benchmarks run at (tests/transcript_scale_util.py; the CPU twin is
tests/test_transcript_scale.py).

  1. One call over 4133 small utterances (device tensors; 29 labels of float64, and 1024 labels of float16) equals, at every
     place, the same utterances in reverse order in calls of 7; equals itself under each forward / find kernel and from host
     arrays; matches numpy at 64 fixed places; gives -inf / None / the empty text at the planted places; and its device results
     are views of one allocation.
  2. ctc_posteriors and ctc_grad_rows over 2.15 GiB of tables in one launch, a posteriors call of 4.3 GiB and an align call of
     1.07 GiB of back-pointers that split under the default budgets, each against the same call in forced small launches and,
     around the 2 GiB (1 GiB) mark, against numpy.
  3. 65538 prefix rows that nothing is launched for: two ctc_prefix_fill launches, live rows on both sides of the boundary."""
import numpy as np
import pytest
import torch

from pyctcdecode_amd import decoder as D
from tests import grad_util, posteriors_util
from tests import transcript_scale_util as U
from tests.align_long_util import same as same_aligned
from tests.align_util import check_aligned, random_logits

pytestmark = pytest.mark.gpu

GPU_PARAMS = ("V29_f64", "V1024_f16")
GiB = 1 << 30


@pytest.fixture(scope="module")
def device_batches():
    made = {}

    def get(name):
        if name not in made:
            b = U.batch_of(name, U.N_GPU)
            made[name] = (b, b.on_device())
        return made[name]

    yield get
    made.clear()


@pytest.mark.parametrize("entry", U.ENTRY_POINTS)
@pytest.mark.parametrize("name", GPU_PARAMS)
def test_wide_batch(name, entry, device_batches, monkeypatch):
    b, dev = device_batches(name)
    assert b.n == 4096 + 37 and len(dev) == b.n and dev[0].is_cuda
    getattr(U.Scale(b, dev, monkeypatch, host=b.xs), entry)()


# ---- part 2 -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table_inputs():
    rng = np.random.default_rng(29)
    return {T: [torch.from_numpy(random_logits(rng, T, U.TABLE_V)).cuda() for _ in range(U.TABLE_INPUTS)]
            for T in (U.TABLE_T, U.BP_T)}


def spread(inputs, n):
    return [inputs[u % len(inputs)] for u in range(n)]


def check_lean_posteriors(dec, got, xin, target, what):
    """A dense=False result of a large call against numpy: its summaries are the bits of the utterance's own dense call, and
    that goes through every check of tests/posteriors_util.py against the numpy forward-backward"""
    alone = dec.posteriors(xin, tokens=target)
    assert got.gamma is None and posteriors_util.same_bits(got, alone, dense=False), what
    x = xin.cpu().numpy()
    posteriors_util.check_posteriors(alone, posteriors_util.yardstick(x, target, U.BLANK), len(x), target, what)


@pytest.mark.parametrize("n", [U.TABLE_UTTS_ONE_LAUNCH, U.TABLE_UTTS_SPLIT], ids=["one_launch_above_2GiB", "splits_at_4GiB"])
def test_posteriors_tables(n, table_inputs):
    per, total, launches, small, small_launches = U.posteriors_plan(n)
    assert (2 * GiB < total <= D.POSTERIORS_TABLE_BUDGET and launches == 1) if n == U.TABLE_UTTS_ONE_LAUNCH else (
        total > D.POSTERIORS_TABLE_BUDGET and launches > U.posteriors_plan(U.TABLE_UTTS_ONE_LAUNCH)[2])
    dec = U.build(U.TABLE_V)
    xin, targets = spread(table_inputs[U.TABLE_T], n), U.table_targets(n, U.TABLE_L)
    got = dec.posteriors_batch(xin, tokens=targets, dense=False)
    assert dec.last_posteriors_launches == launches and dec.last_posteriors_launched == (n, 0), dec.last_posteriors_launches
    forced = dec.posteriors_batch(xin, tokens=targets, dense=False, _table_budget=small)
    assert dec.last_posteriors_launches == small_launches > launches
    differ = [u for u in range(n) if not posteriors_util.same_bits(got[u], forced[u], dense=False)]
    assert not differ, "%d of %d utterances differ from the launches of %d, first %s" % (
        len(differ), n, U.SMALL_LAUNCH_UTTS, differ[:8])
    for u in U.around_mark(per, n, 2 * GiB):
        check_lean_posteriors(dec, got[u], xin[u], targets[u], "posteriors of %d, utt %d" % (n, u))


def test_gradient_reads_tables_above_2gib(table_inputs):
    n = U.TABLE_UTTS_ONE_LAUNCH
    per, total, launches, small, small_launches = U.posteriors_plan(n)
    assert 2 * GiB < total <= D.POSTERIORS_TABLE_BUDGET and launches == 1
    dec = U.build(U.TABLE_V)
    xin, targets = spread(table_inputs[U.TABLE_T], n), U.table_targets(n, U.TABLE_L)
    got = dec.gradient_batch(xin, tokens=targets)
    assert dec.last_gradient_launches == 2 and dec.last_gradient_launched == (n, 0)  # (ctc_posteriors, ctc_grad_rows)
    base = got[0].grad.untyped_storage().data_ptr()
    assert all(g.grad.untyped_storage().data_ptr() == base for g in got)
    forced = dec.gradient_batch(xin, tokens=targets, _table_budget=small)
    assert dec.last_gradient_launches == 2 * small_launches
    differ = [u for u in range(n) if not grad_util.same_bits(got[u], forced[u])]
    assert not differ, "%d of %d utterances differ from the launches of %d, first %s" % (
        len(differ), n, U.SMALL_LAUNCH_UTTS, differ[:8])
    for u in U.around_mark(per, n, 2 * GiB):
        x = xin[u].cpu().numpy()
        grad = grad_util.check_gradient(got[u], grad_util.grad_np(x, targets[u], U.BLANK), x, targets[u], "gradient utt %d" % u,
                                        on_device=True)
        grad_util.check_rows(grad, x, targets[u], U.BLANK, "gradient utt %d" % u)


def test_align_splits_under_the_default_budget(table_inputs):
    n = U.BP_UTTS
    per, total, launches, one = U.align_plan(n)
    assert total > D.ALIGN_BP_BUDGET and launches > 1
    dec = U.build(U.TABLE_V)
    xin, targets = spread(table_inputs[U.BP_T], n), U.table_targets(n, U.BP_L)
    got = dec.align_batch(xin, tokens=targets)
    assert dec.last_align_launches == launches, dec.last_align_launches
    forced = dec.align_batch(xin, tokens=targets, _bp_budget=one)
    assert dec.last_align_launches == n
    differ = [u for u in range(n) if not same_aligned(got[u], forced[u])]
    assert not differ, "%d of %d utterances differ from their own launch, first %s" % (len(differ), n, differ[:8])
    for u in U.around_mark(per, n, D.ALIGN_BP_BUDGET):
        check_aligned(got[u], xin[u].cpu().numpy(), targets[u], dec, None, "align utt %d" % u)


# ---- part 3 -------------------------------------------------------------------------------------------------------------------
def test_dead_prefix_rows():
    xs, prefixes, dead = U.dead_rows_case()
    n_dead = sum(1 for ks in dead for k in ks if k >= 0)
    assert n_dead == U.FILL_PIECE + 3 and 200 <= sum(1 for ks in dead for k in ks if k < 0) <= 400
    dec = U.build(29)
    fills = -(-n_dead // U.FILL_PIECE)
    assert fills == 2
    dev = U.check_dead_rows(dec, [torch.from_numpy(x).cuda() for x in xs], prefixes, dead, fills)
    host = U.check_dead_rows(dec, xs, prefixes, dead, 0)  # (host arrays: the host fills, no launch)
    assert np.array_equal(dev, host)
