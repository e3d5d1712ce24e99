"""Phrase spotting on streams (spot_streams / SpotStreams.feed) on the CPU simulator, which runs ctc_spot_chunk's serial body
(csrc/ctc_align.h, ctc_spot_chunk_seq) over the same spot_ends / spot_step as spot_batch: any cut into chunks against the
whole recording with ==, and against the numpy recursion; the packing; the refusals. The HIP build, through the same
checks: tests/test_gpu_spot_stream.py."""
import pytest

from tests.sim_util import sim_library  # noqa: F401
from tests.spot_stream_util import CUTS, LENGTHS, check_chunked_equals_whole, check_packing, check_refusals


@pytest.mark.parametrize("name", CUTS)
@pytest.mark.parametrize("L", LENGTHS)
def test_chunked_equals_whole_and_numpy(sim_library, L, name):
    check_chunked_equals_whole(L, name)


def test_packing_and_forced_width_agree(sim_library, monkeypatch):
    check_packing(monkeypatch)


def test_refusals(sim_library):
    check_refusals()
