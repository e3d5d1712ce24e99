"""CPU: the prune stage's log-softmax against numpy's own, bit for bit, at label counts on both sides of numpy's 8192-element
summation pieces (csrc/np_sum.h). The simulator's prune stage is built on the header the HIP kernels restate, and the decode
tests see these values only through beam scores at up to 5000 labels."""
import numpy as np
import pytest

from oracle.ctc_oracle import normalise_logits
from tests.sim_util import sim_library  # noqa: F401
from tests.survivor_util import check_exact, numbered_labels, survivors, telling_rows


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("V", [7688, 7689, 8192, 8193, 16385, 65535])
def test_survivor_logps_are_numpys_bits(sim_library, V, dtype):  # noqa: F811
    """Every survivor log-probability == normalise_logits(x) on the matrix in its own dtype, widened to float64, and the
    survivor set is where(lp >= tmin) | {argmax} with no borderline allowance -- at a threshold that prunes, and at one below
    the clip, where every label survives. (7688: the last label count whose pieces have at most 64 leaves; 7689: 65 leaves;
    above 8192: more than one piece.)"""
    from pyctcdecode_amd import build_ctcdecoder

    rng = np.random.default_rng(V + (1 if dtype == np.float64 else 0))
    x = telling_rows(rng, V, dtype)
    lp = normalise_logits(x).astype(np.float64)  # (float32 arithmetic on a float32 matrix; only the clip widens it)
    dec = build_ctcdecoder(numbered_labels(V))
    for tmin in (-6.0, -40.0):
        got = survivors(dec, x, tmin)
        if tmin == -40.0:
            assert all(len(ids) == V for ids, _ in got)
        check_exact(got, lp, tmin, what="V=%d %s tmin=%g" % (V, np.dtype(dtype).name, tmin))
