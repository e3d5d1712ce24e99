"""GPU (-m gpu): greedy best-path decoding (decode_greedy / decode_greedy_batch) on the HIP build -- row_argmax, row_lse_argmax
and greedy_collapse of csrc/ctc_align_hip.hip. The cases of tests/test_greedy.py from host arrays and from device tensors,
device tensors of every dtype read in place at one vocabulary per lanes-per-row choice, at 131 labels (rows off a 16-byte
boundary, elements left over) and through a view one element past an aligned base, planted ties in every dtype, the exact
identities with the HIP align and align_gaps (which pin row_lse_argmax's log-sum-exp to row_lse's bits and its maximum to
row_lse_max's), the cost contract from the kernels' own times, and every case equal to the CPU simulator's."""
import numpy as np
import pytest
import torch

from tests.align_gaps_util import items_of
from tests.align_util import random_logits
from tests.greedy_util import BLANK, VOCABS, build, check_greedy, collapse_np, of_batch, same_batch_entry, same_greedy, tie_rows
from tests.test_greedy import (SEQS, mixed_inputs, run_batch_equals_single_calls, run_collapse, run_family_identities,
                               run_special_rows, run_texts, run_ties)

pytestmark = pytest.mark.gpu

TORCH_DTYPES = (torch.float16, torch.bfloat16, torch.float32, torch.float64)
NP_DTYPES = (np.float16, np.float32, np.float64)


def on_device(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host_of(t):
    """A device tensor as the yardstick sees it: the exact values, in float64 for float64 and in float32 otherwise (the class of
    the probabilities-or-logits test and of the tolerance)."""
    host = t.double().cpu().numpy()
    return host if t.dtype == torch.float64 else host.astype(np.float32)


@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("dtype", NP_DTYPES, ids=lambda d: np.dtype(d).name)
def test_ties_take_the_smaller_index(dtype, V):
    host = run_ties(V, dtype)
    dev = run_ties(V, dtype, on_device)
    assert all(same_greedy(a, b) for a, b in zip(host, dev))


@pytest.mark.parametrize("V", VOCABS)
def test_ties_in_bfloat16_and_off_an_aligned_base(V):
    """bfloat16 (numpy has none) and, for every dtype, the same rows through a view that starts one element past an aligned
    base: element loads in the same grouping, the same labels."""
    dec = build(V)
    for dtype in TORCH_DTYPES:
        x, want = tie_rows(V, torch.empty(0, dtype=dtype).element_size(), np.random.default_rng(V))
        xt = torch.from_numpy(x).to(dtype).cuda()  # (small integers and zeros: exact in every dtype)
        flat = torch.zeros(x.size + 1, dtype=dtype).cuda()
        flat[1:] = xt.reshape(-1)
        tokens = [c for c, _, _ in collapse_np(want, BLANK)]
        for inp in (xt, flat[1:].view(*x.shape)):
            plain = dec.decode_greedy(inp, token_frames=True)
            conf = dec.decode_greedy(inp, confidence="mean")
            assert plain.tokens == tokens, (V, dtype)
            assert conf.tokens == tokens and conf.token_frames == plain.token_frames, (V, dtype)
            check_greedy(conf, host_of(xt), dec, "mean", "%s V=%d" % (dtype, V))


@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("dtype", TORCH_DTYPES, ids=str)
def test_device_tensors(dtype, V):
    """Random rows of every dtype in a ragged batch, one of them through a view one element past an aligned base: the plain
    call (row_argmax) and the confidence call (row_lse_argmax) give the same tokens, both numpy's."""
    dec = build(V)
    rng = np.random.default_rng(V)
    xs = [torch.from_numpy(random_logits(rng, T, V)).to(dtype).cuda() for T in (37, 64, 5, 130)]
    flat = torch.from_numpy(random_logits(rng, 20 * V + 1, 1)[:, 0]).to(dtype).cuda()
    xs.append(flat[1:].view(20, V))
    texts, frames = dec.decode_greedy_batch(xs, token_frames=True)
    ctexts, cframes = dec.decode_greedy_batch(xs, confidence="mean")
    assert texts == ctexts
    for name in ("label", "start", "end", "offsets"):
        assert np.array_equal(getattr(frames, name), getattr(cframes, name)), name
    for u, x in enumerate(xs):
        g = dec.decode_greedy(x, confidence="mean")
        check_greedy(g, host_of(x), dec, "mean", "%s V=%d utt %d" % (dtype, V, u))
        assert same_batch_entry(of_batch(ctexts, cframes, u, dec), g), (dtype, V, u)
        # the family, on the HIP build: exact whatever the ties of a narrow dtype
        a = dec.align(x, tokens=g.tokens, confidence="mean")
        gaps = dec.align_gaps(x, tokens=items_of(g.tokens, [1] * (len(g.tokens) + 1)))
        assert g.score == a.score and g.score == gaps.score, (dtype, V, u, g.score, a.score, gaps.score)


@pytest.mark.parametrize("V", (29, 131))
def test_nan_and_inf_rows(V):
    host = run_special_rows(V)
    dev = run_special_rows(V, on_device)
    assert all(same_greedy(a, b) for a, b in zip(host, dev))


@pytest.mark.parametrize("name", sorted(SEQS))
def test_collapse(name):
    host = run_collapse(name)
    dev = run_collapse(name, on_device)
    assert all(same_greedy(a, b) for a, b in zip(host, dev))


@pytest.mark.parametrize("fold", (None, "mean"))
def test_ragged_batch_list_and_tensor(fold):
    dec, xs, _xin, texts, frames, singles = run_batch_equals_single_calls(on_device, fold)
    _dec, _xs, _xin, htexts, hframes, hsingles = run_batch_equals_single_calls(fold=fold)
    assert texts == htexts and all(same_greedy(a, b) for a, b in zip(singles, hsingles))  # host arrays equal device tensors
    for name in ("label", "start", "end", "offsets", "logp", "score"):
        assert np.array_equal(getattr(frames, name), getattr(hframes, name)), name
    T = max(len(x) for x in xs)
    pad = np.zeros((len(xs), T, 29))
    for u, x in enumerate(xs):
        pad[u, : len(x)] = x
    ctexts, cframes = (dec.decode_greedy_batch(on_device(pad), confidence=fold) if fold
                       else dec.decode_greedy_batch(on_device(pad), token_frames=True))
    for u in range(len(xs)):
        g = dec.decode_greedy(pad[u], token_frames=True, confidence=fold)
        assert same_batch_entry(of_batch(ctexts, cframes, u, dec), g), u


@pytest.mark.parametrize("dtype", NP_DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("V", (29, 131, 1024))
def test_probabilities_and_logits_in_one_batch(V, dtype):
    xs = mixed_inputs(V, dtype)
    *_r, host = run_batch_equals_single_calls(fold="mean", xs=xs, V=V)
    *_r, dev = run_batch_equals_single_calls(on_device, "mean", xs, V)
    assert all(same_greedy(a, b) for a, b in zip(host, dev))
    run_batch_equals_single_calls(on_device, None, xs, V)


def test_texts_of_both_alphabet_kinds():
    host = run_texts()
    dev = run_texts(on_device)
    assert all(same_greedy(a, b) for a, b in zip(host, dev))


@pytest.mark.parametrize("V", VOCABS)
def test_family_identities(V):
    run_family_identities(V, np.float64)
    run_family_identities(V, np.float64, on_device)


@pytest.mark.parametrize("V", VOCABS)
def test_score_identity_under_ties(V):
    run_family_identities(V, np.float16)
    run_family_identities(V, np.float16, on_device)


def test_cost_contract():
    """A plain call classifies nothing and forms no log-sum-exp; a confidence call does both."""
    dec = build(300)
    x = on_device(random_logits(np.random.default_rng(1), 500, 300).astype(np.float32))
    dec.decode_greedy(x)
    ms = dec.last_greedy_timing_ms
    print("plain call: ms", ms, "lse ms", dec.last_greedy_lse_ms)
    assert ms[0] == 0.0 and dec.last_greedy_lse_ms == 0.0 and ms[1] > 0.0 and ms[2] > 0.0 and ms[3] > 0.0
    assert dec.last_greedy_launches == 3
    dec.decode_greedy(x, confidence="mean")
    ms = dec.last_greedy_timing_ms
    print("confidence call: ms", ms, "lse ms", dec.last_greedy_lse_ms)
    assert ms[0] > 0.0 and dec.last_greedy_lse_ms > 0.0 and dec.last_greedy_lse_ms == ms[1] and ms[2] > 0.0
    assert dec.last_greedy_launches == 3


def test_results_equal_the_simulator(monkeypatch):
    """Every case above on the HIP build and on the CPU simulator: integers and texts equal, floats within the float64 bound
    (the two builds' exp and log differ in the last bits)."""
    from pyctcdecode_amd import _binding as B
    from tests.sim.build_sim import build as build_sim

    def run_all():
        out = []
        for V in VOCABS:
            for dtype in NP_DTYPES:
                out += list(run_ties(V, dtype))
            out += run_family_identities(V, np.float64)
        for V in (29, 131):
            out += run_special_rows(V)
            out += run_family_identities(V, np.float16)
        for name in sorted(SEQS):
            out += list(run_collapse(name))
        out += run_texts()
        for fold in (None, "mean"):
            out += run_batch_equals_single_calls(fold=fold)[5]
        for dtype in NP_DTYPES:
            out += run_batch_equals_single_calls(fold="max", xs=mixed_inputs(131, dtype), V=131)[5]
        return out

    hip = run_all()
    monkeypatch.setattr(B, "_LIB", B.Library(build_sim()))
    sim = run_all()
    assert len(hip) == len(sim) > 150
    for k, (a, b) in enumerate(zip(hip, sim)):
        assert a.text == b.text and a.tokens == b.tokens and a.token_frames == b.token_frames and a.text_frames == b.text_frames, k
        assert (a.score is None) == (b.score is None) and (a.token_logp is None) == (b.token_logp is None), k
        if a.score is not None:
            assert abs(a.score - b.score) <= 1e-9, (k, a.score, b.score)
            assert all(abs(p - q) <= 1e-9 for p, q in zip(a.token_logp, b.token_logp)), k
            assert all(abs(p - q) <= 1e-9 for p, q in zip(a.word_logp, b.word_logp)), k
