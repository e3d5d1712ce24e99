"""CPU: beam search at every beam-table size edge (tests/beam_width_util.py) through the simulator, both beam kernels --
the proof that the cases and the oracle agree before a GPU sees them (tests/test_gpu_beam_widths.py runs the same table on the
HIP build). The fullness condition on the cases themselves is asserted here, on the oracle alone."""
import pytest

from tests import beam_width_util as U
from tests.sim_util import sim_library  # noqa: F401

PAIR_IDS = ["%dto%d" % p for p in U.STREAM_PAIRS]


@pytest.mark.parametrize("width", U.WIDTHS)
@pytest.mark.parametrize("name", U.INPUTS)
def test_the_oracle_search_sits_at_the_cut(name, width):
    U.check_fullness(name, width)


@pytest.mark.parametrize("width", U.WIDTHS)
@pytest.mark.parametrize("name", U.INPUTS)
def test_sim_beam_width_edges_vs_oracle(name, width, both_beam_kernels, sim_library):  # noqa: F811
    dec = U.build_decoder(name)
    U.check_case(dec, name, width)
    assert dec.last_beam_kernel == (1 if both_beam_kernels == "wave" and width <= 128 else 2)


@pytest.mark.parametrize("a,b", U.STREAM_PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("name", U.INPUTS)
def test_sim_width_changes_in_a_stream(name, a, b, both_beam_kernels, sim_library):  # noqa: F811
    U.check_stream_pair(U.build_decoder(name), name, a, b)


@pytest.mark.parametrize("a,b", [p for p in U.STREAM_PAIRS if p[0] > p[1]], ids=[i for i, p in zip(PAIR_IDS, U.STREAM_PAIRS) if p[0] > p[1]])
def test_sim_host_imported_beams_at_a_narrower_width(a, b, both_beam_kernels, sim_library):  # noqa: F811
    """More beams than chunk two's beam_width asks for, handed back as a plain list: imported by the host, not refused."""
    U.check_stream_pair(U.build_decoder("words"), "words", a, b, edit=True)


@pytest.mark.parametrize("edit", [False, True], ids=["resident", "hostimport"])
@pytest.mark.parametrize("length", U.SHORT_LENGTHS)
@pytest.mark.parametrize("a,b", U.SHORT_PAIRS, ids=["%dto%d" % p for p in U.SHORT_PAIRS])
@pytest.mark.parametrize("name", U.INPUTS)
def test_sim_short_chunk_behind_a_wider_one(name, a, b, length, edit, both_beam_kernels, sim_library):  # noqa: F811
    """Chunk two of one or three frames: every carried beam is advanced, a text node each, with no later frames to pay for it."""
    U.check_stream_pair(U.build_decoder(name), name, a, b, edit=edit, length=length)


@pytest.mark.parametrize("a,b", U.STREAM_PAIRS, ids=PAIR_IDS)
def test_sim_kernel_after_a_width_change(a, b, both_beam_kernels, sim_library):  # noqa: F811
    """Which kernel ran chunk two (U.WAVE_STREAM_KERNEL): the wave kernel wherever one of its tables holds what came in."""
    dec = U.build_decoder("flat")
    U.check_stream_pair(dec, "flat", a, b)
    assert dec.last_beam_kernel == (U.WAVE_STREAM_KERNEL[(a, b)] if both_beam_kernels == "wave" else 2)


def test_sim_beam_width_257_is_refused(sim_library):  # noqa: F811
    dec = U.build_decoder("flat")
    with pytest.raises(NotImplementedError):
        dec.decode_beams(U.logits("flat"), beam_width=257)
