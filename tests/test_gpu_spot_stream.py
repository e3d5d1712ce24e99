"""GPU (-m gpu): phrase spotting on streams on the HIP build -- ctc_spot_chunk and spot_select of csrc/ctc_align_hip.hip --
through the checks of tests/test_spot_stream.py, then the HIP build against the CPU simulator, and device chunks of every
dtype read in place against host chunks and against spot_batch on the whole recording."""
import numpy as np
import pytest
import torch

from tests.spot_stream_util import (CUTS, LENGTHS, check_chunked_equals_whole, check_packing, check_refusals, cut, length_case,
                                    stream_spots)
from tests.spot_util import SCORE_TOL, check_spot, random_logits, random_target, same
from tests.test_align import build

pytestmark = pytest.mark.gpu


def on_device(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


@pytest.mark.parametrize("name", CUTS)
@pytest.mark.parametrize("L", LENGTHS)
def test_chunked_equals_whole_and_numpy(L, name):
    check_chunked_equals_whole(L, name, on_device)


def test_packing_and_forced_width_agree(monkeypatch):
    check_packing(monkeypatch, on_device)


def test_refusals():
    check_refusals()


def test_hip_against_the_simulator(monkeypatch):
    from pyctcdecode_amd import _binding as B
    from tests.sim.build_sim import build as build_sim

    cases = [length_case(L) for L in (2, 16, 127)]
    hip = [stream_spots(build(29), [x], [[p]], [cut(len(x), "ragged")])[0][0] for p, x in cases]
    monkeypatch.setattr(B, "_LIB", B.Library(build_sim()))
    worst = 0.0
    for (p, x), a in zip(cases, hip):
        b = stream_spots(build(29), [x], [[p]], [cut(len(x), "ragged")])[0][0]
        fin = np.isfinite(b.end_logp)
        assert np.array_equal(np.isfinite(a.end_logp), fin) and abs(a.count - b.count) <= 1e-9 * b.count
        worst = max([worst] + np.abs(a.end_logp[fin] - b.end_logp[fin]).tolist())
    print("HIP against the simulator: worst gap %.2e" % worst)
    assert worst <= SCORE_TOL


@pytest.mark.parametrize("V", [29, 1024])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32, torch.float64])
def test_device_chunks(dtype, V):
    """Two streams, three phrases each, fed in chunks of 9, 0 and the rest; the second stream's rows are a view one element
    past an aligned address. Device chunks equal spot_batch on the whole device tensor and the numpy recursion on its widened
    values; they equal host chunks of the same values too, where numpy has the dtype (bfloat16 has no host form: as float32
    the rows would get float32's row_lse, not bfloat16's)."""
    dec = build(V)
    blank = dec._alphabet.labels.index("")
    rng = np.random.default_rng(V)
    flat = on_device(random_logits(rng, 30 * V + 1, 1)[:, 0]).to(dtype)
    rows = [on_device(random_logits(rng, 37, V)).to(dtype), flat[1:].view(30, V)]
    phrases = []
    for L in (5, 9):
        t = random_target(rng, L, V, doubled=1)
        phrases.append([t, t[:-1], t[1:] + random_target(rng, 1, V)])
    sizes = [[9, 0, 28], [9, 0, 21]]
    whole = dec.spot_batch(rows, tokens=phrases, max_hits=2, trace=True)
    got = stream_spots(dec, rows, phrases, sizes, lambda r: r, max_hits=2)
    host = None
    if dtype != torch.bfloat16:
        host = stream_spots(dec, [r.cpu().numpy() for r in rows], phrases, sizes, max_hits=2)
    for u, cur in enumerate(phrases):
        wide = rows[u].double().cpu().numpy()
        ref = wide if dtype == torch.float64 else wide.astype(np.float32)  # (the widened values are exact)
        for j, p in enumerate(cur):
            assert same(got[u][j], whole[u][j]) and (host is None or same(got[u][j], host[u][j])), (u, j)
            check_spot(got[u][j], ref, p, blank, max_hits=2, what="%s V=%d stream %d phrase %d" % (dtype, V, u, j))
