"""GPU (-m gpu): the frame-prune stage's log-probabilities against numpy's, per kernel route.

float32 rows in the default mode restate the reference's float32 log-softmax (csrc/np_f32.h, csrc/np_sum.h): every survivor's
log-probability must EQUAL numpy's for the float32 matrix, up to 65535 labels -- the decode tests see these values only through
beam scores, at up to 5000 labels, and tests/survivor_util.check_against_cpython allows 1e-9 at best. float64, float16 and
bfloat16 rows are held to their own contracts (see the tests). Matrices are handed over as host arrays (staged at an aligned
address), as device tensors read in place, and as device tensors that start one element past an aligned address."""
import functools
import os

import numpy as np
import pytest

from tests.survivor_util import (as_float64, check_against_cpython, check_exact, expected_logp, numbered_labels, survivors,
                                 telling_rows)
from tests.test_prune_route import BF16, F16, F32, route  # noqa: F401  (the host probe of csrc/prune_route.h)

pytestmark = pytest.mark.gpu

FAST_V = [29, 32, 256, 1020, 1024, 1025, 2048, 2049, 3072, 4095]       # frame_prune_fast (64 rows per wave)
ROW_V = [4096, 5000, 7688, 7689, 8192, 8193, 16385, 65535]            # one wave per row, the generic kernel
PEAKY_TMIN = -5.0
# "every label survives": a threshold below the clip. The per-row kernels keep a row's survivors and their set tables in LDS,
# which holds a whole row of up to 1100 labels; above that the widest threshold the stage admits is used on plain rows instead
# (at most floor(e^6.9) + 2 = 994 survivors, a few hundred in fact)
WHOLE_TMIN, WHOLE_MAX_V = -40.0, 1025
PLAIN_TMIN = -6.9


@functools.lru_cache(maxsize=None)
def _dec(V):
    from pyctcdecode_amd import build_ctcdecoder
    from pyctcdecode_amd import _binding as B

    assert B.get_library().path.endswith("pyctcdecode_amd/libctcdec.so")
    return build_ctcdecoder(numbered_labels(V))


def _rows_for(V):
    return 70 if V <= 4096 else 8  # (two blocks of the 64-rows-per-wave kernel, the second one partial)


def _peaky(rng, T, V):
    """Rows in which one to three labels stand out: at most 15 survive PEAKY_TMIN, which keeps a row inside
    frame_prune_fast (more, and the row is handed to the per-row kernel behind it). float64; the callers narrow it."""
    x = rng.standard_normal((T, V)) * 2.0
    for t in range(T):
        k = 1 + t % 3
        x[t, rng.choice(V, k, replace=False)] += 16.0 + rng.uniform(0, 2, k)
    return x


@functools.lru_cache(maxsize=None)
def _f32_case(V):
    """(peaky matrix, its expected log-probabilities, plain matrix, its expected log-probabilities) -- computed once per V"""
    rng = np.random.default_rng(4000 + V)
    peaky = _peaky(rng, _rows_for(V), V).astype(np.float32)
    plain = telling_rows(rng, V, np.float32, n=min(_rows_for(V), 40))
    lp_peaky, lp_plain = expected_logp(peaky), expected_logp(plain)
    assert int((lp_peaky >= PEAKY_TMIN).sum(axis=1).max()) <= 15
    for a in (peaky, plain, lp_peaky, lp_plain):
        a.setflags(write=False)
    return peaky, lp_peaky, plain, lp_plain


@pytest.mark.parametrize("V", FAST_V + ROW_V)
def test_float32_logps_are_numpys_bits(V, route, monkeypatch):  # noqa: F811
    """float32, default mode: survivor log-probabilities == numpy's for the float32 matrix, sets and order exactly a CPython
    set's, no border rows (with equal bits the threshold test is decidable). Peaky rows stay inside frame_prune_fast up to 4095
    labels; plain rows keep hundreds of labels and go through the per-row kernels (listed behind the fast kernel, or forced by
    CTCDEC_PRUNE_KERNEL=row); up to 1025 labels the per-row kernels also return whole rows.
    Before the 8192-element pieces (csrc/np_sum.h) this failed from 7689 labels on: rows of more than 64 leaves fell back to
    fp64 arithmetic, about 1e-7 from the reference's float32 values."""
    monkeypatch.delenv("CTCDEC_PRUNE_EXP", raising=False)
    monkeypatch.delenv("CTCDEC_PRUNE_KERNEL", raising=False)
    peaky, lp_peaky, plain, lp_plain = _f32_case(V)
    dec = _dec(V)
    r = route(F32, V, n_rows=len(peaky))
    assert r.np and r.kernel == ("fast_f32" if V <= 4095 else "generic"), r
    check_exact(survivors(dec, peaky, PEAKY_TMIN), lp_peaky, PEAKY_TMIN, "V=%d peaky" % V)
    check_exact(survivors(dec, plain, PLAIN_TMIN), lp_plain, PLAIN_TMIN, "V=%d plain" % V)
    monkeypatch.setenv("CTCDEC_PRUNE_KERNEL", "row")
    r = route(F32, V, n_rows=len(peaky), kernel_env="row")
    assert r.np and r.listed == "none" and r.kernel == ("f32x4" if V % 4 == 0 and V <= 1024 else "generic"), r
    check_exact(survivors(dec, plain, PLAIN_TMIN), lp_plain, PLAIN_TMIN, "V=%d plain, per-row kernel" % V)
    if V <= WHOLE_MAX_V:
        got = survivors(dec, peaky, WHOLE_TMIN)
        assert all(len(ids) == V for ids, _ in got)
        check_exact(got, lp_peaky, WHOLE_TMIN, "V=%d whole rows, per-row kernel" % V)
    else:
        check_exact(survivors(dec, peaky, PEAKY_TMIN), lp_peaky, PEAKY_TMIN, "V=%d peaky, per-row kernel" % V)


# ---- float64 ----------------------------------------------------------------------------------------------------------------
# The largest |device - numpy| of a survivor's log-probability, in ulps of the log-probability, over the plain rows of every
# label count up to 7688 below -- measured on the commit before the 8192-element pieces, where the summation order at those
# label counts was numpy's already: 1.00 ulp (at 29, 32, 256, 2048 and 3072 labels; 0 at the nine other label counts up to
# 7688). On that commit 7689, 8193, 16385 and 65535 labels gave 1.00 as well; with the pieces they give 0, 0, 0 and 1.00.
F64_ULPS_MEASURED = 1.0


def _ulps(got, want):
    return np.abs(np.asarray(got) - want) / np.spacing(np.abs(want))


@functools.lru_cache(maxsize=None)
def _f64_case(V):
    rng = np.random.default_rng(8000 + V)
    plain = telling_rows(rng, V, np.float64, n=min(_rows_for(V), 40))
    lp = expected_logp(plain)
    plain.setflags(write=False)
    lp.setflags(write=False)
    return plain, lp


def f64_max_ulps(V):
    plain, lp = _f64_case(V)
    worst = 0.0
    for t, (ids, lps) in enumerate(survivors(_dec(V), plain, PLAIN_TMIN)):
        worst = max(worst, float(_ulps(lps, lp[t][ids]).max()))
    return worst


@pytest.mark.parametrize("V", FAST_V + ROW_V)
def test_float64_logps_within_twice_the_measured_ulps(V, monkeypatch):
    """float64 rows: the device's exp and log are ocml's, not numpy's, so equality is not the contract. Every survivor's
    log-probability is within 2 x F64_ULPS_MEASURED = 2 ulps of numpy's (measured: 1.00 ulp, see there), the sets and their
    order are a CPython set's at 1e-9 (tests/survivor_util.check_against_cpython).
    This bound CANNOT tell summation orders apart at float64: two orders differ in the last bit of the normaliser, which is
    within what ocml's exp and log already differ from numpy's by. The order above 8192 labels is pinned by the float32 test
    above, which runs the same np_order_exp_sum template with T = float."""
    monkeypatch.delenv("CTCDEC_PRUNE_EXP", raising=False)
    monkeypatch.delenv("CTCDEC_PRUNE_KERNEL", raising=False)
    plain, lp = _f64_case(V)
    worst = f64_max_ulps(V)
    print("float64 V=%d: largest |device - numpy| = %.2f ulps of the log-probability" % (V, worst))
    assert worst <= 2 * F64_ULPS_MEASURED, (V, worst)
    assert check_against_cpython(_dec(V), plain, PLAIN_TMIN, 1e-9, lp=lp) < max(1, len(plain) // 20)


# ---- float16 / bfloat16 device tensors ----------------------------------------------------------------------------------------
H_TMIN = -5.0


def _torch_dtype(name):
    import torch

    return {"float16": torch.float16, "bfloat16": torch.bfloat16, "float32": torch.float32}[name]


@functools.lru_cache(maxsize=None)
def _h_case(V, name):
    """A [70, V] matrix of 16-bit logits as a host float32 array holding exactly the 16-bit values: the upper half of the rows at
    scale 4 (about six labels pass H_TMIN: frame_prune_fast keeps them), the lower half at 2.5 (dozens pass: the listed kernel)."""
    import torch

    rng = np.random.default_rng(1600 + V + (7 if name == "bfloat16" else 0))
    x = rng.standard_normal((70, V))
    x[:35] *= 4.0
    x[35:] *= 2.5
    x = torch.from_numpy(x.astype(np.float32)).to(_torch_dtype(name))
    lp = expected_logp(x)
    lp.setflags(write=False)
    return x, lp


def _off_by_one(x):
    """The same matrix on the device, starting one element past an aligned address: flat[1:].view(T, V)"""
    import torch

    flat = torch.empty(x.numel() + 1, dtype=x.dtype, device="cuda")
    assert flat.data_ptr() % 16 == 0
    flat[1:] = x.reshape(-1).to("cuda")
    view = flat[1:].view(x.shape)
    assert view.is_contiguous() and view.data_ptr() % 16 == x.element_size()
    return view


def _h_bound(name, V, aligned):
    """tests/test_gpu_parity._tol: 1e-4 where the 64-rows-per-wave kernel widens 16-bit rows and runs its packed float32
    exponentials (a multiple of eight labels up to 1024, 16-byte aligned rows, not under CTCDEC_PRUNE_EXP=f64), 1e-9 on the
    generic (fp64) path."""
    from tests.test_gpu_parity import _tol

    class Shape:
        dtype, shape = name, (70, V)

    return _tol(Shape)["tol"] if aligned else 1e-9


def _yardstick_border_rows(lp, tmin, tol):
    """Rows of the EXPECTED values in which some label sits within tol of the threshold: what any implementation may count as
    border rows."""
    return int((np.abs(lp - tmin) <= tol).any(axis=1).sum())


@pytest.mark.parametrize("exp_mode", ["np", "f64"])
@pytest.mark.parametrize("name", ["float16", "bfloat16"])
@pytest.mark.parametrize("V,offset", [(256, False), (512, False), (1024, False), (1025, False), (2048, False), (1024, True)])
def test_16_bit_device_tensors(V, offset, name, exp_mode, route, monkeypatch):  # noqa: F811
    """float16 and bfloat16 tensors read in place: 256 / 512 labels (one 16-byte load per lane of frame_prune_fast), 1024 (two),
    1025 and 2048 (the generic kernel), and 1024 labels from an address one element past an aligned one (generic because of the
    base). Expected: the log-softmax of the exact float64 upcast; bounds: _h_bound; order: a real CPython set's; fewer than
    1 row in 20 a border row."""
    if exp_mode == "np":
        monkeypatch.delenv("CTCDEC_PRUNE_EXP", raising=False)
    else:
        monkeypatch.setenv("CTCDEC_PRUNE_EXP", exp_mode)
    monkeypatch.delenv("CTCDEC_PRUNE_KERNEL", raising=False)
    x, lp = _h_case(V, name)
    code = F16 if name == "float16" else BF16
    r = route(code, V, al4=not offset, al16=not offset, n_rows=70, exp=None if exp_mode == "np" else exp_mode)
    packed = V % 8 == 0 and V <= 1024 and not offset and exp_mode == "np"
    assert r.kernel == ("fast_16" if packed else "generic"), r
    tol = _h_bound(name, V, not offset)
    assert tol == (1e-4 if packed else 1e-9)
    assert _yardstick_border_rows(lp, H_TMIN, tol) < 70 // 20
    xd = _off_by_one(x) if offset else x.to("cuda")
    assert check_against_cpython(_dec(V), xd, H_TMIN, tol, lp=lp) < 70 // 20


@pytest.mark.parametrize("name", ["float16", "bfloat16"])
def test_16_bit_rows_from_an_odd_base_equal_the_aligned_ones(name, monkeypatch):
    """Under CTCDEC_PRUNE_KERNEL=row both tensors take the generic kernel: identical ids and bits."""
    monkeypatch.delenv("CTCDEC_PRUNE_EXP", raising=False)
    monkeypatch.setenv("CTCDEC_PRUNE_KERNEL", "row")
    x, _ = _h_case(1024, name)
    assert survivors(_dec(1024), x.to("cuda"), H_TMIN) == survivors(_dec(1024), _off_by_one(x), H_TMIN)


# ---- in place versus staged, float32 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1024, 1020])
def test_float32_in_place_and_staged_rows_give_the_same_bits(V, route, monkeypatch):  # noqa: F811
    """A host array (staged at an aligned address), a device tensor, and the device tensor flat[1:].view(T, V): rows of a
    multiple of four labels read in place from a base that is 4- but not 16-byte aligned take frame_prune_fast<4, 0, false, NP>
    with the generic listed kernel behind it, a pairing no other input reaches. Identical ids and bits, and numpy's."""
    import torch

    monkeypatch.delenv("CTCDEC_PRUNE_EXP", raising=False)
    monkeypatch.delenv("CTCDEC_PRUNE_KERNEL", raising=False)
    r = route(F32, V, al16=False, n_rows=70)
    assert (r.kernel, r.al, r.np, r.listed) == ("fast_f32", False, True, "listed"), r
    peaky, lp_peaky, plain, lp_plain = _f32_case(V)
    for x, lp, tmin in ((peaky, lp_peaky, PEAKY_TMIN), (plain, lp_plain, PLAIN_TMIN)):
        host = survivors(_dec(V), x, tmin)
        xt = torch.from_numpy(np.array(x))
        assert survivors(_dec(V), xt.to("cuda"), tmin) == host
        assert survivors(_dec(V), _off_by_one(xt), tmin) == host
        check_exact(host, lp, tmin, "V=%d" % V)


def test_one_misaligned_utterance_in_a_batch_changes_nothing(monkeypatch):
    """decode_beams_batch over [aligned, off-by-one view, aligned] equals the three single decodes field for field: one
    misaligned utterance changes the whole call's prune route."""
    import torch

    import synth
    from pyctcdecode_amd import build_ctcdecoder

    monkeypatch.delenv("CTCDEC_PRUNE_EXP", raising=False)
    monkeypatch.delenv("CTCDEC_PRUNE_KERNEL", raising=False)
    words = synth.make_words(300, seed=2)
    bpe = synth.make_bpe_vocab(words, size=1023)
    dec = build_ctcdecoder(bpe)
    sentences = synth.make_sentences(words, 40)
    xs = [torch.from_numpy(synth.d_words(4, u, 60, bpe, True, words, sentences, len(bpe), boost=6.0)) for u in range(3)]
    assert all(x.shape[1] == 1024 and x.dtype == torch.float32 for x in xs)
    batch = [xs[0].to("cuda"), _off_by_one(xs[1]), xs[2].to("cuda")]

    def fields(beams):
        return [(b.text, [(w, tuple(f)) for w, f in b.text_frames], b.logit_score, b.lm_score) for b in beams]

    together = dec.decode_beams_batch(None, batch, beam_width=20)
    for u in range(3):
        assert fields(together[u]) == fields(dec.decode_beams(batch[u], beam_width=20)), u
        assert fields(together[u]) == fields(dec.decode_beams(xs[u].to("cuda"), beam_width=20)), u


# ---- planted rows -------------------------------------------------------------------------------------------------------------
def _plant(x, V):
    """The rows of tests/test_gpu_parity.test_hip_rows64_prune_kernel_shapes, in rows 0 .. 5; -> the mask of clean rows"""
    x[0, :] = -np.inf           # an all-masked row
    x[1, 3] = np.inf
    x[2, V // 2] = np.nan
    x[3, : V // 2] = -np.inf    # half the labels masked: a clean row
    x[4, :] = 0.25              # every label ties for the maximum
    x[5, :] = 0.0
    x[5, [V - 1, V // 3]] = 9.0  # two maxima: the first one is the argmax
    good = np.ones(len(x), bool)
    good[[0, 1, 2]] = False
    return good


@pytest.mark.parametrize("V,name", [(1024, "bfloat16"), (8193, "float32")])
def test_planted_rows(V, name, monkeypatch):
    """An all -inf row, a NaN, a +inf, a half-masked row, an all-equal row and a row with two maxima, as bfloat16 at 1024 labels
    (frame_prune_fast<4, 3> hands them to the listed kernel) and as float32 at 8193 labels (more than one summation piece):
    the default route and the per-row kernel give equal lists; the clean rows are numpy's bits (float32) or within the 16-bit
    bounds (bfloat16)."""
    import torch

    monkeypatch.delenv("CTCDEC_PRUNE_EXP", raising=False)
    monkeypatch.delenv("CTCDEC_PRUNE_KERNEL", raising=False)
    T = _rows_for(V)
    rng = np.random.default_rng(77 + V)
    x = (rng.standard_normal((T, V)) * 2.0).astype(np.float32)
    good = _plant(x, V)
    xt = torch.from_numpy(x).to(_torch_dtype(name))  # (0.25, 9.0 and the infinities are exact in bfloat16)
    xd = xt.to("cuda")
    fast = survivors(_dec(V), xd, PEAKY_TMIN)
    monkeypatch.setenv("CTCDEC_PRUNE_KERNEL", "row")
    per_row = survivors(_dec(V), xd, PEAKY_TMIN)
    monkeypatch.delenv("CTCDEC_PRUNE_KERNEL")
    for t in range(T):
        assert fast[t][0] == per_row[t][0], (V, t)
    clean = torch.from_numpy(as_float64(xt)[good]).to(_torch_dtype(name))
    lp = expected_logp(clean)
    assert lp[1][0] == lp[1][V - 1] and int(np.argmax(lp[2])) == V // 3  # (the all-equal row, the two maxima)
    if name == "float32":
        check_exact([fast[t] for t in np.flatnonzero(good)], lp, PEAKY_TMIN, "V=%d planted" % V)
        assert [per_row[t] for t in np.flatnonzero(good)] == [fast[t] for t in np.flatnonzero(good)]
    else:
        tol = _h_bound(name, V, True)
        assert check_against_cpython(_dec(V), clean.to("cuda"), PEAKY_TMIN, tol, lp=lp) < max(1, int(good.sum()) // 20)
        for t in np.flatnonzero(good):
            np.testing.assert_allclose(fast[t][1], per_row[t][1], rtol=0, atol=2 * tol)
