"""Beam ORDER against the reference, strictly (north star: "beam ordering bit-exact").

* For float64 input the frame-prune stage sums the log-softmax normaliser in numpy's own order (np.sum is pairwise:
  csrc/np_sum.h), so a frame's log-probabilities are the reference's bit for bit wherever exp / log round like numpy's --
  and then every golden case comes back in exactly the reference's order, runs of exactly equal scores included
  (the simulator build: all 58; the HIP build: see the `-m gpu` twin and the session summary line "strict order").
* Where an order can still differ (exp / log of another math library rounding the last bit the other way), it can only
  be a case whose order the reference ITSELF does not keep under such a change: oracle/order_vs_rounding.py."""
import numpy as np
import pytest

from tests.golden_util import load_cases, lm_path
from tests.sim_util import sim_library  # noqa: F401

CASES, INPUTS = load_cases()
F64 = [c for c in CASES if INPUTS[c["input"]].dtype == np.float64]


def _ids(beams):
    return [(b.text, [[w, int(a), int(z)] for w, (a, z) in b.text_frames]) for b in beams]


def _strict_differences(build_ctcdecoder, to_input):
    bad = []
    for case in F64:
        dec = build_ctcdecoder(case["labels"], lm_path(case["lm"]), case["unigrams"], **case["build"])
        out = dec.decode_beams(to_input(INPUTS[case["input"]]), **case["decode"])
        if _ids(out) != [(e["text"], e["frames"]) for e in case["expected"]]:
            bad.append(case["name"])
    return bad


def test_sim_returns_every_float64_golden_case_in_exactly_the_reference_order(sim_library, both_beam_kernels):  # noqa: F811
    from pyctcdecode_amd import build_ctcdecoder

    assert _strict_differences(build_ctcdecoder, lambda x: x) == []


def test_cases_whose_order_hinges_on_the_last_bit_are_unstable_in_the_reference_itself():
    """The four cases in which round 3's kernels (normaliser summed in another order) returned another order. Run on the
    staged reference (oracle/_ref) where there is one, else on its restatement oracle/ctc_oracle.py, which the golden vectors
    pin to the reference's beams and order (tests/test_oracle_golden.py): both name the same float64 golden cases."""
    from oracle import make_ref
    from oracle.order_vs_rounding import unstable_cases, unstable_cases_oracle

    suspects = ["toy_nolm_16beams", "toy_history_prune", "toy_lm_unk0_prune20", "toy_lm_autounigrams_prune60"]
    stable_sample = ["libri_char", "toy_lm_default"]
    names = [c["name"] for c in CASES]
    run = unstable_cases if make_ref.available() else unstable_cases_oracle
    got = run(names=[n for n in suspects + stable_sample if n in names])
    assert sorted(got) == sorted(suspects)


@pytest.mark.gpu
def test_hip_order_differences_are_confined_to_rounding_unstable_cases(both_beam_kernels):
    """On the device exp / log are ocml's, not glibc's: an order may still differ -- but only in a case whose order the
    reference itself does not keep when the last bit of a log-probability changes."""
    import torch

    from pyctcdecode_amd import build_ctcdecoder

    bad = _strict_differences(build_ctcdecoder, lambda x: torch.from_numpy(x).cuda())
    print("strict order differences on the device [%s]: %s" % (both_beam_kernels, bad or "none"))
    assert set(bad) <= {"toy_nolm_16beams", "toy_history_prune", "toy_lm_unk0_prune20", "toy_lm_autounigrams_prune60"}
