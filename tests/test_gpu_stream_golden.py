"""GPU (-m gpu): the HIP build's partial_decode_beams / partial_decode_beams_batch against goldens of the UNMODIFIED reference
(tests/golden/cases_stream.json.gz; scenarios and what is compared: tests/test_stream_golden.py, tests/stream_golden_util.py).
Every scenario under both beam kernels, fed once from host arrays and once from device tensors; the out-of-phase streams in one
launch per step; BASELINE configs[0] taken literally.

Bounds: check_beams' defaults for float64 chunks, tests.test_gpu_parity._tol(x) for float32 ones. Only tests/golden/ and synth
are read."""
import numpy as np
import pytest

from tests import stream_golden_util as U
from tests.golden_util import check_beams

pytestmark = pytest.mark.gpu

STREAMS = U.scenarios("stream")
PHASES = [s for s in STREAMS if len(s["streams"]) > 1]
UNREAD = [s for s in STREAMS if not all(st["read"] for stream in s["streams"] for st in stream["steps"])]
CONFIG0 = U.scenarios("decode")


def _name(s):
    return s["name"]


def _build():
    from pyctcdecode_amd import build_ctcdecoder

    return build_ctcdecoder


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


FEEDS = {"host": lambda a: a, "device": _dev}


def _bounds(scenario):
    """float32 chunks: the device's float32 bound; everything else check_beams' defaults"""
    from tests.test_gpu_parity import _tol

    dtypes = {st["dtype"] for stream in scenario["streams"] for st in stream["steps"]}
    if dtypes == {"float64"}:
        return {}
    assert dtypes == {"float32"}, dtypes
    V = len(U.labels_of(scenario["labels"], U.FIXTURE)[0]) + 1
    return _tol(np.empty((0, V), dtype=np.float32))


def _check_all(got, scenario, what):
    n = 0
    for u, (steps, stream) in enumerate(zip(got, scenario["streams"])):
        n += U.check_steps(steps, stream, "expected", what="%s %s[%d]" % (what, scenario["name"], u), **_bounds(scenario))
    return n


def _native():
    from tests.test_gpu_parity import _loaded_native

    _loaded_native()


@pytest.mark.parametrize("feed", sorted(FEEDS))
@pytest.mark.parametrize("scenario", STREAMS, ids=_name)
def test_hip_equals_the_reference_stream(scenario, feed, both_beam_kernels):
    _native()
    got = U.run_scenario(_build(), FEEDS[feed], scenario)
    n = _check_all(got, scenario, "hip %s %s" % (both_beam_kernels, feed))
    if all(st["read"] for stream in scenario["streams"] for st in stream["steps"]):
        assert n == sum(len(stream["steps"]) for stream in scenario["streams"])  # every step was compared


@pytest.mark.parametrize("feed", sorted(FEEDS))
@pytest.mark.parametrize("scenario", UNREAD, ids=_name)
def test_hip_unread_stream_step_by_step(scenario, feed, both_beam_kernels):
    """The unread route leaves nothing to compare before the end: replay it once per step and look at that step alone."""
    for k in range(len(scenario["streams"][0]["steps"]) - 1):
        got = U.run_scenario(_build(), FEEDS[feed], scenario, read_step=k)
        assert got[0][k] is not None
        _check_all(got, scenario, "hip %s %s look at %d" % (both_beam_kernels, feed, k))


@pytest.mark.parametrize("feed", sorted(FEEDS))
@pytest.mark.parametrize("scenario", PHASES, ids=_name)
def test_hip_streams_out_of_phase_in_one_launch(scenario, feed, both_beam_kernels):
    got = U.run_scenario(_build(), FEEDS[feed], scenario, batched=True)
    assert _check_all(got, scenario, "hip batched %s %s" % (both_beam_kernels, feed)) == sum(
        len(stream["steps"]) for stream in scenario["streams"])


@pytest.mark.parametrize("feed", sorted(FEEDS))
@pytest.mark.parametrize("case", CONFIG0, ids=_name)
def test_hip_config0_literal(case, feed, both_beam_kernels):
    from tests.test_gpu_parity import _tol

    _native()
    labels, _ = U.labels_of(case["labels"])
    x = U.checked_input(case["input"], labels, False).astype(case["dtype"])
    dec = _build()(labels)
    assert dec.decode(FEEDS[feed](x), **case["decode"]) == case["text"]
    out = dec.decode_beams(FEEDS[feed](x), **case["decode"])
    check_beams([(o.text, o.text_frames, o.logit_score, o.lm_score) for o in out], case["expected"],
                what="hip %s %s %s" % (both_beam_kernels, feed, case["name"]), **_tol(x))
