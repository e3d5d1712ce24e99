"""GPU (-m gpu): phrase spotting (spot / spot_batch) on the HIP build -- ctc_spot and ctc_spot_wave of csrc/ctc_align_hip.hip --
through the checks of tests/test_spot.py, then the wave kernel against the group kernel float for float, device tensors of
every dtype read in place, and the HIP build against the CPU simulator."""
import numpy as np
import pytest
import torch

from tests.spot_util import SCORE_TOL, check_spot, random_logits, random_target, same
from tests.test_align import build
from tests.test_spot import LENGTH_IDS, LENGTHS, TINY, check_enumeration, check_length_case, check_ragged_batch

pytestmark = pytest.mark.gpu


def on_device(x):
    return torch.from_numpy(x).cuda()


@pytest.mark.parametrize("V,T", TINY)
def test_the_event_by_enumeration(V, T):
    check_enumeration(V, T)


@pytest.mark.parametrize("case", LENGTHS, ids=LENGTH_IDS)
def test_against_numpy(case):
    check_length_case(case, on_device)  # (a device tensor: read in place; the untraced call inside takes the host array)


def test_wave_kernel_equals_group_kernel(monkeypatch):
    short = [(c, name) for c, name in zip(LENGTHS, LENGTH_IDS) if c[0] <= 127]
    got = {}
    for kernel in ("wave", "group"):
        monkeypatch.setenv("CTCDEC_FIND_KERNEL", kernel)
        dec = build(29)
        for (L, T, phrase, x), name in short:
            got[kernel, name] = dec.spot(x, tokens=[phrase, phrase[:1], phrase[-2:]], max_hits=64, trace=True)
            assert dec.last_spot_launched == ((3, 0) if kernel == "wave" else (0, 3)), (kernel, name)
    for _, name in short:
        assert all(same(a, b) for a, b in zip(got["wave", name], got["group", name])), name
    # `wave` is a preference: 128 labels still take the group kernel, and one call launches both
    L, T, phrase, x = next(c for c in LENGTHS if c[0] == 128 and c[1] == 300)
    monkeypatch.setenv("CTCDEC_FIND_KERNEL", "wave")
    both = dec.spot(on_device(x), tokens=[phrase, phrase[:127], phrase[:3]], max_hits=2, trace=True)
    assert dec.last_spot_launched == (2, 1) and dec.last_spot_launches == 2
    for p, g in zip([phrase, phrase[:127], phrase[:3]], both):
        assert same(g, dec.spot(x, tokens=[p], max_hits=2, trace=True)[0]), len(p)
    assert dec.last_spot_launched == (1, 0)


@pytest.mark.parametrize("V", [29, 131, 1024])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32, torch.float64])
def test_device_tensors(dtype, V):
    """Rows that are and are not 16-byte aligned, three phrases per utterance, and a view one element past an aligned address."""
    dec = build(V)
    blank = dec._alphabet.labels.index("")
    rng = np.random.default_rng(V)
    xs, phrases = [], []
    for T, L in ((37, 5), (64, 9), (5, 2)):
        xs.append(on_device(random_logits(rng, T, V)).to(dtype))
        t = random_target(rng, L, V, doubled=1)
        phrases.append([t, t[:-1], t[1:] + random_target(rng, 1, V)])
    flat = on_device(random_logits(rng, 20 * V + 1, 1)[:, 0]).to(dtype)
    xs.append(flat[1:].view(20, V))
    t = random_target(rng, 6, V)
    phrases.append([t, t[:3], t[:1]])
    got = dec.spot_batch(xs, tokens=phrases, max_hits=2, trace=True)
    for u, (x, cur) in enumerate(zip(xs, phrases)):
        host = x.double().cpu().numpy()
        ref = host if dtype == torch.float64 else host.astype(np.float32)  # (the widened values are exact)
        for j, p in enumerate(cur):
            check_spot(got[u][j], ref, p, blank, max_hits=2, what="%s V=%d utt %d phrase %d" % (dtype, V, u, j))


def test_ragged_batch_equals_singles_host_input_and_the_simulator(monkeypatch):
    from pyctcdecode_amd import _binding as B
    from tests.sim.build_sim import build as build_sim

    xs, phrases, batch = check_ragged_batch(on_device)
    host = build(29).spot_batch(xs, tokens=phrases, max_hits=3, trace=True)
    assert all(same(a, b) for cur_a, cur_b in zip(batch, host) for a, b in zip(cur_a, cur_b))
    monkeypatch.setattr(B, "_LIB", B.Library(build_sim()))
    sim = build(29).spot_batch(xs, tokens=phrases, max_hits=3, trace=True)
    worst = 0.0
    for a, b in ((a, b) for cur_a, cur_b in zip(batch, sim) for a, b in zip(cur_a, cur_b)):
        fin = np.isfinite(b.end_logp)
        assert np.array_equal(np.isfinite(a.end_logp), fin) and abs(a.count - b.count) <= 1e-9 * b.count
        worst = max([worst] + np.abs(a.end_logp[fin] - b.end_logp[fin]).tolist())
    print("HIP against the simulator: worst gap %.2e" % worst)
    assert worst <= SCORE_TOL  # (2.3e-13 when written, not 0: DESIGN.md, "Phrase spotting")
