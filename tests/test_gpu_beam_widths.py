"""GPU (-m gpu): beam search at every beam-table size edge (tests/beam_width_util.py) on the HIP build, device tensors --
beam_wave<64|100|128> under a forced wave kernel, beam_decode<32|64|128|256> at 256 and at 512 threads (candidate chunks of 512
and, up to the 128 table at 512 threads, 1024) under a forced workgroup kernel. Full beam lists: the cut behind the
beam_width-th beam is taken in nearly every frame (the condition itself: tests/test_beam_widths.py). The oracle's results are
computed once per case and shared by the three kernel settings."""
import pytest

from tests import beam_width_util as U

pytestmark = pytest.mark.gpu

KERNELS = (("wave", None), ("group", "256"), ("group", "512"))
PAIR_IDS = ["%dto%d" % p for p in U.STREAM_PAIRS]


@pytest.fixture(params=KERNELS, ids=["wave", "group256", "group512"])
def kernel(request, monkeypatch):
    forced, threads = request.param
    monkeypatch.setenv("CTCDEC_BEAM_KERNEL", forced)
    if threads is None:
        monkeypatch.delenv("CTCDEC_GROUP_THREADS", raising=False)
    else:
        monkeypatch.setenv("CTCDEC_GROUP_THREADS", threads)
    return forced


def _dev(a):
    import torch

    return torch.tensor(a, device="cuda")  # (a copy: the cases' arrays are read-only)


def _native():
    from pyctcdecode_amd import _binding as B

    lib = B.get_library()
    assert lib.path.endswith("pyctcdecode_amd/libctcdec.so"), lib.path


@pytest.mark.parametrize("width", U.WIDTHS)
@pytest.mark.parametrize("name", U.INPUTS)
def test_hip_beam_width_edges_vs_oracle(name, width, kernel):
    _native()
    dec = U.build_decoder(name)
    U.check_case(dec, name, width, _dev)
    assert dec.last_beam_kernel == (1 if kernel == "wave" and width <= 128 else 2)


@pytest.mark.parametrize("a,b", U.STREAM_PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("name", U.INPUTS)
def test_hip_width_changes_in_a_stream(name, a, b, kernel):
    _native()
    U.check_stream_pair(U.build_decoder(name), name, a, b, _dev)


@pytest.mark.parametrize("a,b", [p for p in U.STREAM_PAIRS if p[0] > p[1]], ids=[i for i, p in zip(PAIR_IDS, U.STREAM_PAIRS) if p[0] > p[1]])
def test_hip_host_imported_beams_at_a_narrower_width(a, b, kernel):
    """More beams than chunk two's beam_width asks for, handed back as a plain list: imported by the host, not refused."""
    _native()
    U.check_stream_pair(U.build_decoder("words"), "words", a, b, _dev, edit=True)


@pytest.mark.parametrize("edit", [False, True], ids=["resident", "hostimport"])
@pytest.mark.parametrize("length", U.SHORT_LENGTHS)
@pytest.mark.parametrize("a,b", U.SHORT_PAIRS, ids=["%dto%d" % p for p in U.SHORT_PAIRS])
@pytest.mark.parametrize("name", U.INPUTS)
def test_hip_short_chunk_behind_a_wider_one(name, a, b, length, edit, kernel):
    """Chunk two of one or three frames: every carried beam is advanced, a text node each, with no later frames to pay for it."""
    _native()
    U.check_stream_pair(U.build_decoder(name), name, a, b, _dev, edit=edit, length=length)


@pytest.mark.parametrize("a,b", U.STREAM_PAIRS, ids=PAIR_IDS)
def test_hip_kernel_after_a_width_change(a, b, kernel):
    """Which kernel ran chunk two (U.WAVE_STREAM_KERNEL): the wave kernel wherever one of its tables holds what came in."""
    _native()
    dec = U.build_decoder("flat")
    U.check_stream_pair(dec, "flat", a, b, _dev)
    assert dec.last_beam_kernel == (U.WAVE_STREAM_KERNEL[(a, b)] if kernel == "wave" else 2)


def test_hip_beam_width_257_is_refused():
    _native()
    dec = U.build_decoder("flat")
    with pytest.raises(NotImplementedError):
        dec.decode_beams(_dev(U.logits("flat")), beam_width=257)
