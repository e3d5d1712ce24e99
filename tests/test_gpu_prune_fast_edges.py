"""GPU (-m gpu): the edges of frame_prune_fast (csrc/frame_prune_hip.hip), the 64-rows-per-wave prune kernel.

Everything goes through ctcdec_frame_survivors (tests/survivor_util.survivors). float32 rows in the default mode: survivor ids,
their order (a real CPython set's), their count and the bits of every log-probability equal numpy's (check_exact). The shapes
are the smallest at which the kernel takes another path: blocks of 1, 63, 64, 65 and 129 rows; rows that fill every lane's
loads (1024 labels) and rows that end inside one (32, 128, 1020) or need element-wise loads (1025); candidates crowded into one
lane or spread one per lane; 15, 16 and 17 of them (the hand-over to the per-row kernel); ties for the maximum; a label exactly
at the threshold; the bounds of the exponential's fast form (a minimum 87 below the maximum); rows the kernel must hand over
(-inf masks, NaN) between ordinary ones. Every planted matrix asserts on the CPU that numpy sees the shape the case names."""
import functools

import numpy as np
import pytest

from tests.survivor_util import check_against_cpython, check_exact, expected_logp, numbered_labels, survivors

pytestmark = pytest.mark.gpu

TMIN = -5.0
V0 = 1024
# csrc/frame_prune_hip.hip: a candidate is a label at or above  xthr - 3e-5 (4 + |xthr|)  in float32, xthr = the threshold on the
# logits; with the maximum at 0 and log(sum) < 3 that margin is at least 3e-5 * (4 + 2) = 1.8e-4 and at most 3e-5 * 9 = 2.7e-4
NEAR = 1.0e-4      # a near miss: this far below the threshold -- inside the screen's margin, outside the exact test


@functools.lru_cache(maxsize=None)
def _dec(V):
    from pyctcdecode_amd import build_ctcdecoder

    return build_ctcdecoder(numbered_labels(V))


def _clear(monkeypatch):
    monkeypatch.delenv("CTCDEC_PRUNE_EXP", raising=False)
    monkeypatch.delenv("CTCDEC_PRUNE_KERNEL", raising=False)


def _peaky(rng, T, V, scale=2.0):
    """Rows in which one to three labels stand out (at most a handful pass TMIN: the rows stay inside frame_prune_fast)"""
    x = rng.standard_normal((T, V)) * scale
    for t in range(T):
        k = 1 + t % 3
        x[t, rng.choice(V, k, replace=False)] += 16.0 + rng.uniform(0, 2, k)
    return x.astype(np.float32)


def _exact(x, tmin, what, V=None):
    lp = expected_logp(x)
    check_exact(survivors(_dec(V or x.shape[1]), x, tmin), lp, tmin, what)
    return lp


@functools.lru_cache(maxsize=None)
def _rows_case():
    x = _peaky(np.random.default_rng(71), 129, V0)
    lp = expected_logp(x)
    assert int((lp >= TMIN).sum(axis=1).max()) <= 15
    x.setflags(write=False)
    lp.setflags(write=False)
    return x, lp


@pytest.mark.parametrize("T", [1, 63, 64, 65, 129])
def test_row_counts(T, monkeypatch):
    """partial blocks, the first and the last row of a wave, a third block of one row"""
    _clear(monkeypatch)
    x, lp = _rows_case()
    # (the LAST T rows: row 128 is the first row of the third block at T = 129 and the only row at T = 1)
    check_exact(survivors(_dec(V0), np.array(x[129 - T:]), TMIN), lp[129 - T:], TMIN, "T=%d" % T)


@pytest.mark.parametrize("V", [32, 128, 1020, 1024, 1025])
def test_label_counts(V, monkeypatch):
    """one and four loads per lane, rows that end inside a load (32, 1020), one leaf (128), the element-wise loads (1025)"""
    _clear(monkeypatch)
    x = _peaky(np.random.default_rng(900 + V), 70, V)
    lp = _exact(x, TMIN, "V=%d" % V)
    assert int((lp >= TMIN).sum(axis=1).max()) <= 15


def _flat(T, V=V0, level=-12.0, seed=5):
    """Background rows: every label near `level` (distinct values), nothing near the threshold once something stands at 0"""
    rng = np.random.default_rng(seed)
    return (level + rng.uniform(-1.0, 1.0, (T, V))).astype(np.float32)


def _lane_labels(lane):
    """the sixteen labels lane `lane` holds of a 1024-label float32 row: four consecutive ones from each of its four loads"""
    return [(k * 64 + lane) * 4 + e for k in range(4) for e in range(4)]


def test_survivors_inside_one_lane(monkeypatch):
    """2 .. 15 survivors, all among one lane's sixteen labels (lanes 0, 5 and 63), the other 63 lanes without a candidate"""
    _clear(monkeypatch)
    rows = []
    for lane in (0, 5, 63):
        for n in (2, 7, 15):
            row = _flat(1, seed=lane * 16 + n)[0]
            row[_lane_labels(lane)[:n]] = np.linspace(0.0, -2.0, n, dtype=np.float32)
            rows.append(row)
    x = np.stack(rows)
    lp = _exact(x, TMIN, "one lane")
    for t, (lane, n) in enumerate((lane, n) for lane in (0, 5, 63) for n in (2, 7, 15)):
        assert sorted(np.flatnonzero(lp[t] >= TMIN)) == sorted(_lane_labels(lane)[:n])


def _spread(n_surv, n_near, seed):
    """A 1024-label row with n_surv survivors, one per lane (lanes 2, 5, 8, ...), and n_near labels NEAR below the threshold,
    one per lane further on: the survivors in [-2, 0], the near misses placed by numpy's own float32 log-softmax"""
    row = _flat(1, seed=seed)[0]
    lanes = [2 + 3 * j for j in range(n_surv + n_near)]
    ids = [_lane_labels(lane)[(5 * j) % 16] for j, lane in enumerate(lanes)]
    row[ids[:n_surv]] = np.linspace(0.0, -2.0, n_surv, dtype=np.float32)
    near = ids[n_surv:]
    for _ in range(4):  # (the near misses move the normaliser by ~1e-3 of itself: settle them in a few rounds)
        lp = expected_logp(row[None, :])[0]
        lse = -float(lp[ids[0]])  # (the maximum is 0: its log-probability is -log(sum))
        row[near] = np.float32(lse + TMIN - NEAR)
    return row, ids[:n_surv], near


@pytest.mark.parametrize("n_surv,n_near", [(15, 1), (15, 2), (14, 2), (14, 3), (16, 0), (15, 0)])
def test_candidates_one_per_lane(n_surv, n_near, monkeypatch):
    """Sixteen candidates of which fifteen survive stay in the kernel (15 + 1, 14 + 2); seventeen candidates (15 + 2, 14 + 3)
    and sixteen survivors (16 + 0) go to the per-row kernel behind it; 15 + 0 is the plain boundary. Each candidate in a lane
    of its own, so that the column fills in lane order. The outputs are numpy's either way."""
    _clear(monkeypatch)
    rows, want = [], []
    for seed in range(3):
        row, surv, near = _spread(n_surv, n_near, 100 * n_surv + 10 * n_near + seed)
        rows.append(row)
        want.append((surv, near))
    x = np.stack([_peaky(np.random.default_rng(3), 1, V0)[0]] + rows + [_peaky(np.random.default_rng(4), 1, V0)[0]])
    lp = _exact(x, TMIN, "%d survivors + %d near misses" % (n_surv, n_near))
    for t, (surv, near) in enumerate(want, start=1):
        assert sorted(np.flatnonzero(lp[t] >= TMIN)) == sorted(surv), t
        below = np.flatnonzero((lp[t] < TMIN) & (lp[t] >= TMIN - 1.8e-4))  # inside the screen's margin whatever xthr is
        assert sorted(below) == sorted(near), (t, lp[t][near])


@pytest.mark.parametrize("n", [15, 16])
def test_fifteen_and_sixteen_survivors(n, monkeypatch):
    """the boundary the kernel's comment states as "more than 16 candidates / 15 survivors": survivors scattered at random"""
    _clear(monkeypatch)
    rng = np.random.default_rng(160 + n)
    x = _flat(6, seed=n)
    for t in range(6):
        x[t, rng.choice(V0, n, replace=False)] = np.linspace(0.0, -2.5, n, dtype=np.float32)
    lp = _exact(x, TMIN, "%d survivors" % n)
    assert ((lp >= TMIN).sum(axis=1) == n).all()


@pytest.mark.parametrize("ties", [2, 3])
def test_equal_maxima(ties, monkeypatch):
    """Two and three exactly equal maxima: numpy.argmax is the first one. Rows 0 - 2: the maxima pass the threshold (they are
    all candidates, phase B picks the smallest id); rows 3 - 5: nothing passes (a flat row: the kernel searches the lane masks
    of `== max`), ties in one lane, in one group of four across lanes, and in different loads of different lanes."""
    _clear(monkeypatch)
    places = [[_lane_labels(9)[3], _lane_labels(9)[8], _lane_labels(9)[15]],
              [_lane_labels(40)[5], _lane_labels(7)[5], _lane_labels(63)[5]],
              [_lane_labels(50)[0], _lane_labels(3)[14], _lane_labels(20)[6]]]
    x = np.concatenate([_flat(3, seed=31), _flat(3, level=0.0, seed=32)])
    for t in range(6):
        x[t, places[t % 3][:ties]] = np.float32(0.0 if t < 3 else 1.5)
    lp = _exact(x, TMIN, "%d equal maxima" % ties)
    for t in range(6):
        assert int(np.argmax(lp[t])) == min(places[t % 3][:ties])
        assert int((lp[t] >= TMIN).sum()) == (ties if t < 3 else 0), t


def test_label_exactly_at_the_threshold(monkeypatch):
    """token_min_logp = a label's float32 log-probability, widened: it survives (>=); one float64 ulp above it, it does not --
    the two thresholds are the same float32 number, only the fp64 test of phase B tells them apart"""
    _clear(monkeypatch)
    x = _peaky(np.random.default_rng(12), 8, V0)
    x[:, 100] = x.max(axis=1) - np.float32(4.75)  # a label that ends near -5
    lp = expected_logp(x)
    at = float(lp[2][100])
    above = float(np.nextafter(at, 0.0))
    assert -5.5 < at < -4.5 and np.float32(at) == np.float32(above) and at < above
    got_at, got_above = survivors(_dec(V0), x, at), survivors(_dec(V0), x, above)
    check_exact(got_at, lp, at, "at the threshold")
    check_exact(got_above, lp, above, "one ulp above")
    assert 100 in got_at[2][0] and 100 not in got_above[2][0]


def test_maximum_in_the_first_and_the_last_element(monkeypatch):
    """the maximum in element 0 (lane 0, first load) and in element 1023 (lane 63, last load): alone, and with a tie"""
    _clear(monkeypatch)
    x = _flat(4, seed=8)
    x[0, 0] = x[1, V0 - 1] = 0.0
    x[2, [0, V0 - 1]] = 0.0
    x[3, V0 - 1] = 0.0
    x[3, V0 - 2] = -1.0
    lp = _exact(x, TMIN, "first / last element")
    assert [int(np.argmax(r)) for r in lp] == [0, V0 - 1, 0, V0 - 1]


def test_minimum_at_the_route_boundary(monkeypatch):
    """A row whose smallest logit is 86.5 below its maximum stays in the kernel (exponentials without the underflow rules), one
    at 87.0 and one at 87.5 below go to the per-row kernel: numpy's bits on both sides. The smallest logit in the first, a
    middle and the last lane."""
    _clear(monkeypatch)
    rows = []
    for gap in (86.5, 87.0, 87.5):
        for at in (0, 517, V0 - 1):
            row = _peaky(np.random.default_rng(int(gap * 2) + at), 1, V0)[0]
            row[at] = row.max() - np.float32(gap)
            assert float(row.max() - row.min()) == gap
            rows.append(row)
    _exact(np.stack(rows), TMIN, "minimum 86.5 / 87 / 87.5 below the maximum")


def test_masked_and_nan_rows_between_ordinary_ones(monkeypatch):
    """Rows with -inf masks and a row with a NaN, each between ordinary rows of the same wave: the kernel hands them to the per-row
    kernel and the neighbours are untouched. Clean rows (the masked ones included): numpy's bits; the NaN row: what the per-row
    kernel gives for it on its own route (CTCDEC_PRUNE_KERNEL=row)."""
    _clear(monkeypatch)
    x = np.array(_rows_case()[0][:70])
    x[10, 5::7] = -np.inf
    x[11, :512] = -np.inf
    x[30, 700] = np.nan
    x[63, 3] = -np.inf     # (the last row of the first wave)
    x[64, 1000] = np.nan   # (the first row of the second)
    fast = survivors(_dec(V0), x, TMIN)
    clean = [t for t in range(70) if t not in (30, 64)]
    lp = expected_logp(x[clean])
    assert np.isfinite(lp).all()
    check_exact([fast[t] for t in clean], lp, TMIN, "masked rows")
    monkeypatch.setenv("CTCDEC_PRUNE_KERNEL", "row")
    per_row = survivors(_dec(V0), x, TMIN)
    for t in (30, 64):
        assert fast[t][0] == per_row[t][0], t
        np.testing.assert_array_equal(np.asarray(fast[t][1]), np.asarray(per_row[t][1]))
    assert [per_row[t] for t in clean] == [fast[t] for t in clean]


@functools.lru_cache(maxsize=None)
def _sixteen_bit_case(name):
    import torch

    rng = np.random.default_rng(2100 + len(name))
    x = rng.standard_normal((70, V0)) * 4.0  # (about six labels pass TMIN: the rows stay in the kernel)
    xt = torch.from_numpy(x.astype(np.float32)).to({"float16": torch.float16, "bfloat16": torch.bfloat16}[name])
    lp = expected_logp(xt)
    lp.setflags(write=False)
    return xt, lp


@pytest.mark.parametrize("name", ["float16", "bfloat16"])
def test_sixteen_bit_rows(name, monkeypatch):
    """the same matrix as float16 and bfloat16 device tensors at 1024 labels (frame_prune_fast<4, 2 / 3>), against the bound of
    those inputs (tests/test_gpu_parity._tol: 1e-4) and the log-softmax of the exact upcast"""
    from tests.test_gpu_parity import _tol

    _clear(monkeypatch)
    xt, lp = _sixteen_bit_case(name)

    class Shape:
        dtype, shape = name, (70, V0)

    tol = _tol(Shape)["tol"]
    assert tol == 1e-4
    assert int((np.abs(lp - TMIN) <= tol).any(axis=1).sum()) < 70 // 20
    assert check_against_cpython(_dec(V0), xt.to("cuda"), TMIN, tol, lp=lp) < 70 // 20


@pytest.mark.parametrize("V", [1020, 1024, 1025])
def test_polynomial_mode(V, monkeypatch):
    """CTCDEC_PRUNE_EXP=pk (frame_prune_fast<4, 0, AL, false>): the polynomial exponentials, held to that mode's 1e-4"""
    _clear(monkeypatch)
    monkeypatch.setenv("CTCDEC_PRUNE_EXP", "pk")
    x = _peaky(np.random.default_rng(300 + V), 70, V)
    lp = expected_logp(x)
    assert int((np.abs(lp - TMIN) <= 1e-4).any(axis=1).sum()) < 70 // 20
    assert check_against_cpython(_dec(V), x, TMIN, 1e-4, lp=lp) < 70 // 20
