"""CPU: the streaming calls against goldens of the UNMODIFIED reference's get_starting_state / partial_decode_beams
(tests/golden/cases_stream.json.gz, written by oracle/make_golden_stream.py): every LMBeam -- text, next_word, partial_word,
last_char, text_frames, partial_frames, logit_score, lm_score -- after EVERY step of every scenario, for the oracle and for the
package on the simulator under both beam kernels. tests/test_gpu_stream_golden.py replays the same on the HIP build.

Bounds: tests.golden_util.check_beams' defaults (1e-9 absolute on both scores, order exact outside runs of reference scores
within 1e-9), float32 chunks included: the oracle keeps the input dtype like the reference, and the simulator restates numpy's
float32 log-softmax.

Hot words that change in mid-stream (hot_change*, hot_dropped*): the goldens hold the reference as it is (`expected_stale`:
memoised texts and partial words keep the OLD set's bonus) and the reference whose caller refreshes its memos at the change
(`expected`). The oracle is the former and, after OracleState.refresh_memos, the latter; the package is the latter."""
import numpy as np
import pytest

from tests import stream_golden_util as U
from tests.golden_util import check_beams
from tests.sim_util import sim_library  # noqa: F401

STREAMS = U.scenarios("stream")
CHANGING = [s for s in STREAMS if s["two_expectations"]]
PHASES = [s for s in STREAMS if len(s["streams"]) > 1]
UNREAD = [s for s in STREAMS if not all(st["read"] for stream in s["streams"] for st in stream["steps"])]
CONFIG0 = U.scenarios("decode")


def _name(s):
    return s["name"]


def _build():
    from pyctcdecode_amd import build_ctcdecoder

    return build_ctcdecoder


def _check_all(got, scenario, which, what):
    for u, (steps, stream) in enumerate(zip(got, scenario["streams"])):
        U.check_steps(steps, stream, which, what="%s %s[%d]" % (what, scenario["name"], u))


def test_fixture_holds_the_scenarios_it_should():
    names = sorted(_name(s) for s in STREAMS)
    assert len(names) == 18 and len(CHANGING) == 5 and len(PHASES) == 3 and [_name(s) for s in UNREAD] == ["bpe_force_unread"]
    assert [_name(s) for s in CONFIG0] == ["config0_literal"]
    for s in CHANGING:  # the two expectations differ: the scenario can tell the contracts apart
        assert any(a != b for st in s["streams"] for a, b in zip(st["expected"], st["expected_stale"]))
    for s in STREAMS:
        for st in s["streams"]:
            assert len(st["expected"]) == len(st["steps"]) and all(len(b) > 0 for b in st["expected"])


@pytest.mark.parametrize("scenario", STREAMS, ids=_name)
def test_oracle_equals_the_reference_stream(scenario):
    """The oracle as it stands: the reference itself, stale hot-word memos included."""
    which = "expected_stale" if scenario["two_expectations"] else "expected"
    _check_all(U.run_oracle(scenario, refresh=False), scenario, which, "oracle")


@pytest.mark.parametrize("scenario", CHANGING, ids=_name)
def test_oracle_with_refreshed_memos_equals_the_refreshed_reference(scenario):
    _check_all(U.run_oracle(scenario, refresh=True), scenario, "expected", "oracle+refresh")


@pytest.mark.parametrize("scenario", STREAMS, ids=_name)
def test_sim_equals_the_reference_stream(scenario, sim_library, both_beam_kernels):  # noqa: F811
    _check_all(U.run_scenario(_build(), lambda a: a, scenario), scenario, "expected", "sim " + both_beam_kernels)


@pytest.mark.parametrize("scenario", UNREAD, ids=_name)
def test_sim_unread_stream_step_by_step(scenario, sim_library, both_beam_kernels):  # noqa: F811
    """The unread route leaves nothing to compare before the end: replay it once per step and look at that step alone."""
    for k in range(len(scenario["streams"][0]["steps"]) - 1):
        got = U.run_scenario(_build(), lambda a: a, scenario, read_step=k)
        assert got[0][k] is not None and all(g is None for j, g in enumerate(got[0][:-1]) if j != k)
        _check_all(got, scenario, "expected", "sim %s look at %d" % (both_beam_kernels, k))


@pytest.mark.parametrize("scenario", PHASES, ids=_name)
def test_sim_streams_out_of_phase_in_one_launch(scenario, sim_library, both_beam_kernels):  # noqa: F811
    """One partial_decode_beams_batch call per step: empty and one-frame chunks beside long ones, processed_frames that differ
    per stream. (The reference ran the streams one after another.)"""
    _check_all(U.run_scenario(_build(), lambda a: a, scenario, batched=True), scenario, "expected",
               "sim batched " + both_beam_kernels)


def _config0_input(case):
    labels, _ = U.labels_of(case["labels"])
    return labels, U.checked_input(case["input"], labels, False).astype(case["dtype"])


@pytest.mark.parametrize("case", CONFIG0, ids=_name)
def test_oracle_config0_literal(case):
    from oracle.ctc_oracle import build_oracle
    from pyctcdecode_amd.alphabet import Alphabet

    labels, x = _config0_input(case)
    alpha = Alphabet.build_alphabet(labels)
    orc = build_oracle(alpha.labels, alpha.is_bpe)
    with np.errstate(all="ignore"):
        assert orc.decode(x, **case["decode"]) == case["text"]
        out = orc.decode_beams(x, **case["decode"])
    check_beams([(o[0], o[2], o[3], o[4]) for o in out], case["expected"], what="oracle " + case["name"])


@pytest.mark.parametrize("case", CONFIG0, ids=_name)
def test_sim_config0_literal(case, sim_library, both_beam_kernels):  # noqa: F811
    labels, x = _config0_input(case)
    dec = _build()(labels)
    assert dec.decode(x, **case["decode"]) == case["text"]
    out = dec.decode_beams(x, **case["decode"])
    check_beams([(o.text, o.text_frames, o.logit_score, o.lm_score) for o in out], case["expected"],
                what="sim %s %s" % (both_beam_kernels, case["name"]))
