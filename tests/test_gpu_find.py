"""GPU (-m gpu): phrase search (find / find_batch) on the HIP build -- ctc_find and ctc_find_wave of csrc/ctc_align_hip.hip. The
shape and planted cases of tests/test_find.py against the same numpy recursion and selection from host arrays and device
tensors, device tensors of every dtype read in place, the wave kernel against the group kernel float for float and window
for window, one call that launches both, every hit against align on its own window, and the HIP build against the CPU
simulator."""
import numpy as np
import pytest
import torch

from tests.find_util import (SCORE_TOL, WAVE_MAX_LABELS, case_input, check_found, feasible, neg_inf_case, random_logits,
                             random_target, windows_of, yardstick)
from tests.test_align import build
from tests.test_find import PLANTED, SHAPES, WHOLE_MATRIX, planted_case, ragged_phrases, same

pytestmark = pytest.mark.gpu

SHORT = [c for c in SHAPES if len(c[3]) <= WAVE_MAX_LABELS]


@pytest.mark.parametrize("case", SHAPES, ids=[c[0] for c in SHAPES])
def test_shape_cases(case):
    name, V, T, target, _dtype, _kind = case
    dec = build(V)
    x = case_input(case)
    blank = dec._alphabet.labels.index("")
    a = dec.find(x, tokens=[target], max_hits=3, trace=True)[0]  # (a host array: staged)
    assert dec.last_find_launched == ((1, 0) if len(target) <= WAVE_MAX_LABELS else (0, 1))
    b = dec.find(torch.from_numpy(x).cuda(), tokens=[target], max_hits=3, trace=True)[0]  # (a device tensor: read in place)
    check_found(a, x, target, blank, max_hits=3, what=name + " host")
    assert same(a, b), name
    assert len(a.hits) >= 1
    if name in WHOLE_MATRIX:
        assert windows_of(a) == [(0, T)], (name, a.hits)


def test_no_frames_too_few_frames_and_neg_inf_logits():
    dec = build(29)
    got = dec.find(torch.zeros((0, 29), dtype=torch.float64).cuda(), tokens=[[2, 3], [4]], trace=True)
    assert [g.hits for g in got] == [[], []] and dec.last_find_launched == (0, 0)
    short = torch.from_numpy(random_logits(np.random.default_rng(3), 5, 29)).cuda()
    got = dec.find(short, tokens=[[9, 6, 13, 13, 16]], trace=True)[0]
    assert got.hits == [] and dec.last_find_launched == (0, 0) and np.all(got.end_logp == -np.inf) and np.all(got.end_start == -1)
    x, phrase = neg_inf_case()
    a = dec.find(x, tokens=[phrase], max_hits=3, trace=True)[0]
    b = dec.find(torch.from_numpy(x).cuda(), tokens=[phrase], max_hits=3, trace=True)[0]
    check_found(a, x, phrase, 0, max_hits=3, what="-inf logits")
    assert same(a, b) and a.hits


@pytest.mark.parametrize("n_occ,max_hits", PLANTED, ids=["%d_planted_%d_hits" % c for c in PLANTED])
def test_planted_phrases(n_occ, max_hits):
    dec = build(29)
    x, phrase, windows = planted_case(n_occ)
    a = dec.find(x, tokens=[phrase], max_hits=max_hits, trace=True)[0]
    b = dec.find(torch.from_numpy(x).cuda(), tokens=[phrase], max_hits=max_hits, trace=True)[0]
    ref = check_found(a, x, phrase, 0, max_hits=max_hits, what="%d planted, max_hits %d" % (n_occ, max_hits))
    assert same(a, b)
    assert windows_of(a) == [(s, e) for s, e, _ in yardstick(x, phrase, 0, max_hits)[0]]
    first = windows_of(a)[:n_occ]
    assert set(first) <= set(windows) and len(first) == min(n_occ, max_hits), (first, windows)
    assert np.array_equal(a.end_start, ref[1])


@pytest.mark.parametrize("V", [29, 131, 1024])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32, torch.float64])
def test_device_tensors(dtype, V):
    """Rows of every dtype, at vocabularies whose rows are and are not 16-byte aligned, three phrases per utterance, and a
    view whose base is one element past an aligned address."""
    dec = build(V)
    blank = dec._alphabet.labels.index("")
    rng = np.random.default_rng(V)
    xs, phrases = [], []
    for T, L in ((37, 5), (64, 9), (5, 2)):
        xs.append(torch.from_numpy(random_logits(rng, T, V)).to(dtype).cuda())
        t = random_target(rng, L, V, doubled=1)
        phrases.append([t, t[:-1], t[1:] + random_target(rng, 1, V)])
    flat = torch.from_numpy(random_logits(rng, 20 * V + 1, 1)[:, 0]).to(dtype).cuda()
    xs.append(flat[1:].view(20, V))  # (contiguous, but its base is one element past an aligned address)
    t = random_target(rng, 6, V)
    phrases.append([t, t[:3], t[:1]])
    got = dec.find_batch(xs, tokens=phrases, max_hits=2, trace=True)
    for u, (x, cur) in enumerate(zip(xs, phrases)):
        host = x.double().cpu().numpy()
        ref = host if dtype == torch.float64 else host.astype(np.float32)  # (the widened values are exact)
        for j, p in enumerate(cur):
            check_found(got[u][j], ref, p, blank, max_hits=2, what="%s V=%d utt %d phrase %d" % (dtype, V, u, j))


def test_wave_kernel_equals_group_kernel(monkeypatch):
    """Every case the wave kernel takes (L = 31, 32 and 127 put states across the lane and wave edges; 64 hits fill the lanes
    that hold the windows taken), under each kernel forced in turn: the floats, the windows and the traces are equal, and
    last_find_launched shows which kernel took them."""
    jobs = [(c[1], case_input(c), [c[3]], 3, c[0]) for c in SHORT]
    for n_occ in (1, 2, 3):
        x, phrase, _ = planted_case(n_occ)
        jobs.append((29, x, [phrase, phrase[:2], phrase[-1:]], 64, "%d planted" % n_occ))
    got = {}
    for kernel in ("wave", "group"):
        monkeypatch.setenv("CTCDEC_FIND_KERNEL", kernel)
        for V, x, phrases, max_hits, name in jobs:
            dec = build(V)
            got[kernel, name] = dec.find(x, tokens=phrases, max_hits=max_hits, trace=True)
            n = sum(1 for p in phrases if feasible(len(x), p))
            assert dec.last_find_launched == ((n, 0) if kernel == "wave" else (0, n)), (kernel, name, dec.last_find_launched)
    for V, x, phrases, max_hits, name in jobs:
        assert all(same(a, b) for a, b in zip(got["wave", name], got["group", name])), name
        blank = build(V)._alphabet.labels.index("")
        for p, g in zip(phrases, got["wave", name]):
            check_found(g, x, p, blank, max_hits=max_hits, what=name)


def test_one_call_launches_both_kernels(monkeypatch):
    dec = build(29)
    rng = np.random.default_rng(6)
    x = random_logits(rng, 600, 29)
    phrases = [random_target(rng, L, 29, doubled=min(2, L // 2)) for L in (3, 127, 128, 40, 260, 1, 520)]
    dev = torch.from_numpy(x).cuda()
    got = dec.find(dev, tokens=phrases, max_hits=2, trace=True)
    assert dec.last_find_launched == (4, 3) and dec.last_find_launches == 2
    for p, g in zip(phrases, got):
        assert same(dec.find(x, tokens=[p], max_hits=2, trace=True)[0], g), len(p)
        check_found(g, x, p, 0, max_hits=2, what="L=%d" % len(p))
    monkeypatch.setenv("CTCDEC_FIND_KERNEL", "wave")  # (a preference: the long phrases still take the group kernel)
    again = dec.find(dev, tokens=phrases, max_hits=2, trace=True)
    assert dec.last_find_launched == (4, 3) and all(same(a, b) for a, b in zip(got, again))
    monkeypatch.setenv("CTCDEC_FIND_KERNEL", "group")
    again = dec.find(dev, tokens=phrases, max_hits=2, trace=True)
    assert dec.last_find_launched == (0, 7) and all(same(a, b) for a, b in zip(got, again))


def test_a_hit_is_the_alignment_of_its_window():
    """hit.logp is, bit for bit, what align returns for the phrase on the hit's own frames: the sums run in the same order."""
    dec = build(29)
    n = 0
    for n_occ in (1, 2, 3):
        x, phrase, windows = planted_case(n_occ)
        dev = torch.from_numpy(x).cuda()
        found = dec.find(dev, tokens=[phrase], max_hits=n_occ)[0]
        assert sorted(windows_of(found)) == sorted(windows)
        for h in found.hits:
            a = dec.align(dev[h.start:h.end], tokens=phrase)
            assert a.score == h.logp, (n_occ, h, a.score)
            assert a.path[0] == phrase[0] and a.path[-1] == phrase[-1]
            n += 1
    c = next(c for c in SHAPES if c[0] == "L129_T300")
    x = case_input(c)
    h = dec.find(x, tokens=[c[3]])[0].hits[0]
    assert dec.align(x[h.start:h.end], tokens=c[3]).score == h.logp
    assert n == 6


def test_ragged_batch_equals_singles_and_the_simulator(monkeypatch):
    from pyctcdecode_amd import _binding as B
    from tests.sim.build_sim import build as build_sim

    dec = build(29)
    xs, phrases = ragged_phrases()
    dev = [torch.from_numpy(x).cuda() for x in xs]
    batch = dec.find_batch(dev, tokens=phrases, max_hits=3, trace=True)
    assert dec.last_find_launched == (11, 1)
    for u, cur in enumerate(phrases):
        assert all(same(a, b) for a, b in zip(batch[u], dec.find(dev[u], tokens=cur, max_hits=3, trace=True))), u
    split = dec.find_batch(dev, tokens=phrases, max_hits=3, trace=True, _trace_budget=12 * 300)
    assert dec.last_find_launches > 2
    assert all(same(a, b) for cur_a, cur_b in zip(batch, split) for a, b in zip(cur_a, cur_b))
    monkeypatch.setattr(B, "_LIB", B.Library(build_sim()))
    sim = build(29).find_batch(xs, tokens=phrases, max_hits=3, trace=True)
    worst = 0.0
    for u, (cur_a, cur_b) in enumerate(zip(batch, sim)):
        for a, b in zip(cur_a, cur_b):
            fin = np.isfinite(b.end_logp)
            assert np.array_equal(np.isfinite(a.end_logp), fin), u
            if fin.any():
                worst = max(worst, float(np.max(np.abs(a.end_logp[fin] - b.end_logp[fin]))))
            assert len(a.hits) == len(b.hits), u
            for p, q in zip(a.hits, b.hits):
                assert abs(p.logp - q.logp) <= SCORE_TOL, (u, p, q)
    print("HIP against the simulator: worst gap %.2e" % worst)
    assert worst <= SCORE_TOL
