"""GPU (-m gpu): streaming token frames and confidences on the HIP build -- surv_ledger_append keeps every pushed frame's
survivors on the device, token_logp_ledger<FOLD> folds a token's frames out of it. The scenarios are those of
tests/test_stream_tokens.py (tests/stream_tokens_scenarios.py), fed device tensors (and once host chunks)."""
import numpy as np
import pytest

from tests import stream_tokens_scenarios as S

pytestmark = pytest.mark.gpu


def _build():
    from pyctcdecode_amd import build_ctcdecoder

    return build_ctcdecoder


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("beam_width,labels,is_bpe", S.ALPHABETS, ids=S.ALPHABET_IDS)
def test_hip_unread_chunks_then_the_end(beam_width, labels, is_bpe, both_beam_kernels):
    S.scenario_unread_then_end(_build(), _dev, beam_width, labels, is_bpe)


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_hip_unread_chunks_low_precision_input(dtype):
    S.scenario_unread_then_end(_build(), _dev, 100, S.BPE, True, dtype=dtype)


def test_hip_unread_chunks_from_host_memory():
    S.scenario_unread_then_end(_build(), lambda a: a, 40, S.ALPHABETS[0][1], False)


@pytest.mark.parametrize("beam_width,labels,is_bpe", S.ALPHABETS, ids=S.ALPHABET_IDS)
def test_hip_chunking_does_not_change_the_numbers(beam_width, labels, is_bpe):
    S.scenario_chunking_changes_nothing(_build(), _dev, beam_width, labels, is_bpe)


@pytest.mark.parametrize("beam_width,labels,is_bpe", S.ALPHABETS, ids=S.ALPHABET_IDS)
def test_hip_mid_stream_reads(beam_width, labels, is_bpe, both_beam_kernels):
    S.scenario_mid_stream_reads(_build(), _dev, beam_width, labels, is_bpe)


@pytest.mark.parametrize("beam_width", [8, 100])
def test_hip_batch_of_streams(beam_width):
    S.scenario_batch_of_streams(_build(), _dev, beam_width)


@pytest.mark.parametrize("beam_width,labels,is_bpe", S.ALPHABETS, ids=S.ALPHABET_IDS)
def test_hip_force_next_word_on_a_middle_chunk(beam_width, labels, is_bpe):
    S.scenario_force_next_word(_build(), _dev, beam_width, labels, is_bpe)


@pytest.mark.parametrize("beam_width,labels,is_bpe", S.ALPHABETS, ids=S.ALPHABET_IDS)
def test_hip_probability_like_chunks(beam_width, labels, is_bpe):
    S.scenario_probabilities(_build(), _dev, beam_width, labels, is_bpe)


def test_hip_refusals_leave_the_previous_lists_readable(monkeypatch):
    S.scenario_refusals(_build(), _dev, monkeypatch)


@pytest.mark.parametrize("beam_width,labels,is_bpe", S.ALPHABETS, ids=S.ALPHABET_IDS)
def test_hip_nothing_for_those_who_do_not_ask(beam_width, labels, is_bpe):
    S.scenario_nothing_for_those_who_do_not_ask(_build(), _dev, beam_width, labels, is_bpe)
