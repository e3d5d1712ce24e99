"""The CPU twin of tests/test_gpu_transcript_scale.py: the harness of tests/transcript_scale_util.py on the simulator, so that
the harness itself -- inputs, planted places, the comparison of one large call with small ones, the routes, the numpy checks --
is checked without a GPU. N_SIM = 301 utterances under the planting rules of the GPU test. The float16 batch has 131 labels
here, not the GPU test's 1024: the simulator walks every column of the 300-frame utterances in one thread, and 1024 of them
take it ten seconds a call; what the narrow dtype changes in the harness (the widened reference, the float32-class bounds) is
the same at 131.

Part 3 (more than 65535 prefix rows that nothing is launched for) runs at full count: the simulator takes host arrays, whose
rows the host fills. Part 2's table sizes are asserted from the planning functions alone, with no allocation."""
import pytest

from pyctcdecode_amd import decoder as D
from tests import transcript_scale_util as U
from tests.sim_util import sim_library  # noqa: F401

SIM_PARAMS = ("V29_f64", "V131_f16")


def test_places():
    for n in (U.N_SIM, U.N_GPU):
        t0, bad, long = U.planted(n)
        assert len(t0) >= 8 and len(bad) >= 8 and len(long) == 5 and t0[0] == 0 and t0[-1] == n - 1
        places = U.sample_places(n)
        assert places == U.sample_places(n) and len(places) == 64 and {0, n - 1} <= set(places) and set(long) <= set(places)
        for p in t0 + bad:
            assert {q for q in (p - 1, p + 1) if 0 <= q < n} <= set(places), p
        for m in (256, 512, 768, 1024):
            assert m >= n or {m - 1, m, m + 1} <= set(places)
    assert U.N_GPU == 4096 + 37 and all(U.N_GPU % k for k in (4, 16, 64, 256)) and U.N_GPU > 256 * 16


@pytest.mark.parametrize("name", SIM_PARAMS)
def test_batch_follows_the_planting_rules(name):
    b = U.batch_of(name, U.N_SIM)
    V, dtype, max_t = U.PARAMS[name]
    assert b.n == U.N_SIM and all(x.shape == (T, V) and x.dtype == dtype for x, T in zip(b.xs, b.frames))
    assert [b.frames[u] for u in b.t0] == [0] * 8 and [b.frames[u] for u in b.long] == [300] * 5
    assert sorted(len(b.targets[u]) for u in b.long) == [127, 127, 128, 129, 129]
    assert all(not U.feasible(b.frames[u], b.targets[u]) for u in b.bad)
    planted = set(b.t0 + b.bad + b.long)
    for u in range(b.n):
        if u not in planted:
            assert 1 <= b.frames[u] <= max_t and len(b.targets[u]) <= min(b.frames[u], 12) and U.feasible(b.frames[u], b.targets[u])
        assert len(b.items[u]) == len(b.phrases[u]) <= 4 and all(b.phrases[u]) and len(b.gap_targets[u]) >= 1
    assert any(a == c for t in b.targets for a, c in zip(t, t[1:]))  # (doubled labels)
    assert b.n_items % 2 == 1 and {len(cur) for cur in b.items} >= {0, 1, 2, 3}
    assert b.n // 3 <= sum(1 for f in b.gap_flags if any(f)) <= 2 * b.n // 3
    assert U.batch_of(name, U.N_SIM) is b


@pytest.mark.parametrize("entry", U.ENTRY_POINTS)
@pytest.mark.parametrize("name", SIM_PARAMS)
def test_wide_batch(name, entry, sim_library, monkeypatch):  # noqa: F811
    b = U.batch_of(name, U.N_SIM)
    getattr(U.Scale(b, b.xs, monkeypatch), entry)()


def test_dead_prefix_rows(sim_library):  # noqa: F811
    """Part 3 at full count, from host arrays: the rows nothing is launched for are the host's to fill."""
    xs, prefixes, dead = U.dead_rows_case()
    flat = [k for ks in dead for k in ks]
    assert sum(1 for k in flat if k >= 0) == U.FILL_PIECE + 3 and 200 <= sum(1 for k in flat if k < 0) <= 400
    U.check_dead_rows(U.build(29), xs, prefixes, dead, None)


def test_table_plans():
    """Part 2 without an allocation: the utterance counts, the bytes, and the side of each budget they fall on."""
    GiB = 1 << 30
    assert D.POSTERIORS_TABLE_BUDGET == 4 * GiB and D.ALIGN_BP_BUDGET == GiB
    per, total, launches, small, small_launches = U.posteriors_plan(U.TABLE_UTTS_ONE_LAUNCH)
    assert per == 32 * U.TABLE_T * 128 == 2 << 20 and 2 * GiB < total <= D.POSTERIORS_TABLE_BUDGET and launches == 1
    assert small == U.SMALL_LAUNCH_UTTS * per and small_launches == -(-U.TABLE_UTTS_ONE_LAUNCH // U.SMALL_LAUNCH_UTTS)
    assert U.around_mark(per, U.TABLE_UTTS_ONE_LAUNCH, 2 * GiB) == [0, 1023, 1024, 1025, U.TABLE_UTTS_ONE_LAUNCH - 1]
    assert total - 1024 * per > 0 and 1024 * per == 2 * GiB  # (utterance 1024's table starts at 2 GiB: 32 bits of bytes end there)
    per, total, launches, small, small_launches = U.posteriors_plan(U.TABLE_UTTS_SPLIT)
    assert total > D.POSTERIORS_TABLE_BUDGET and launches == 2 and small_launches == -(-U.TABLE_UTTS_SPLIT // U.SMALL_LAUNCH_UTTS)
    per, total, launches, one = U.align_plan(U.BP_UTTS)
    assert per == U.BP_T * 512 == 1 << 20 and total > D.ALIGN_BP_BUDGET and launches == 2 and one == per
    assert U.launches_under([per] * U.BP_UTTS, one) == U.BP_UTTS
    assert U.launches_under([3, 0, 3, 3, 0, 7], 7) == 3 and U.launches_under([0, 0], 7) == 0


def test_launch_model_is_the_librarys(sim_library):  # noqa: F811
    """launches_under, from which the GPU test takes the launch counts it demands, against the launches the library makes
    under small budgets."""
    b = U.batch_of("V29_f64", U.N_SIM)
    dec = U.build(b.V)
    idx = [u for u in range(40, 90) if u not in b.bad]
    sizes = [dec._state_table_bytes(b.frames[u], len(b.targets[u])) for u in idx]
    for budget in (max(sizes), 3 * max(sizes), sum(sizes) // 2, sum(sizes)):
        dec.posteriors_batch(U.sub(b.xs, idx), tokens=U.sub(b.targets, idx), dense=False, _table_budget=budget)
        want = U.launches_under(sizes, budget)
        # (the 300-frame utterance's table is the largest; every target is short: one kernel launch per launch of the call)
        assert dec.last_posteriors_launches == want, (budget, dec.last_posteriors_launches, want)
    sizes = [dec._bp_table_bytes(b.frames[u], len(b.targets[u])) for u in idx]
    for budget in (max(sizes), sum(sizes) // 3, sum(sizes)):
        dec.align_batch(U.sub(b.xs, idx), tokens=U.sub(b.targets, idx), _bp_budget=budget)
        assert dec.last_align_launches == U.launches_under(sizes, budget), budget
