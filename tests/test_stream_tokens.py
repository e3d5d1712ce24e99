"""Streaming token frames and confidences (partial_decode_beams(..., token_frames=True / confidence=...)): CPU checks through
the simulator build, whose api.cpp runs the bodies of csrc/surv_ledger.h in loops. tests/test_gpu_stream_tokens.py runs the same
scenarios (tests/stream_tokens_scenarios.py) on the HIP build."""
import numpy as np
import pytest

from tests import stream_tokens_scenarios as S
from tests.sim_util import sim_library  # noqa: F401


def _build():
    from pyctcdecode_amd import build_ctcdecoder

    return build_ctcdecoder


def _as_is(a):
    return a


@pytest.mark.parametrize("beam_width,labels,is_bpe", S.ALPHABETS, ids=S.ALPHABET_IDS)
def test_unread_chunks_then_the_end(beam_width, labels, is_bpe, sim_library, both_beam_kernels):  # noqa: F811
    S.scenario_unread_then_end(_build(), _as_is, beam_width, labels, is_bpe)


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_unread_chunks_low_precision_input(dtype, sim_library):  # noqa: F811
    S.scenario_unread_then_end(_build(), _as_is, 100, S.BPE, True, dtype=dtype)


@pytest.mark.parametrize("beam_width,labels,is_bpe", S.ALPHABETS, ids=S.ALPHABET_IDS)
def test_chunking_does_not_change_the_numbers(beam_width, labels, is_bpe, sim_library):  # noqa: F811
    S.scenario_chunking_changes_nothing(_build(), _as_is, beam_width, labels, is_bpe)


@pytest.mark.parametrize("beam_width,labels,is_bpe", S.ALPHABETS, ids=S.ALPHABET_IDS)
def test_mid_stream_reads(beam_width, labels, is_bpe, sim_library, both_beam_kernels):  # noqa: F811
    S.scenario_mid_stream_reads(_build(), _as_is, beam_width, labels, is_bpe)


@pytest.mark.parametrize("beam_width", [8, 100])
def test_batch_of_streams(beam_width, sim_library):  # noqa: F811
    S.scenario_batch_of_streams(_build(), _as_is, beam_width)


@pytest.mark.parametrize("beam_width,labels,is_bpe", S.ALPHABETS, ids=S.ALPHABET_IDS)
def test_force_next_word_on_a_middle_chunk(beam_width, labels, is_bpe, sim_library):  # noqa: F811
    S.scenario_force_next_word(_build(), _as_is, beam_width, labels, is_bpe)


@pytest.mark.parametrize("beam_width,labels,is_bpe", S.ALPHABETS, ids=S.ALPHABET_IDS)
def test_probability_like_chunks(beam_width, labels, is_bpe, sim_library):  # noqa: F811
    S.scenario_probabilities(_build(), _as_is, beam_width, labels, is_bpe)


def test_refusals_leave_the_previous_lists_readable(sim_library, monkeypatch):  # noqa: F811
    S.scenario_refusals(_build(), _as_is, monkeypatch)


@pytest.mark.parametrize("beam_width,labels,is_bpe", S.ALPHABETS, ids=S.ALPHABET_IDS)
def test_nothing_for_those_who_do_not_ask(beam_width, labels, is_bpe, sim_library):  # noqa: F811
    S.scenario_nothing_for_those_who_do_not_ask(_build(), _as_is, beam_width, labels, is_bpe)
