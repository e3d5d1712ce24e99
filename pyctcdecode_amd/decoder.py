"""Drop-in Python surface of the decoder (reference: pyctcdecode/decoder.py).

Same names, positional order and defaults as the reference for ``build_ctcdecoder``,
``BeamSearchDecoderCTC.decode / decode_beams / decode_batch / decode_beams_batch``, the frozen
dataclasses ``Beam / LMBeam / OutputBeam`` and ``reset_params / cleanup / clear_class_models``.
All decoding work happens in libctcdec (HIP, gfx950) through ctypes; this file only marshals.
The ``pool`` argument of the batch entry points is accepted for signature compatibility and
ignored: a batch is one device launch (one workgroup per utterance) instead of a process pool.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import itertools
import logging
import math
import os
import threading
from typing import Any, Collection, Dict, Iterable, List, Optional, Sequence, Tuple, TypeVar

import numpy as np

from . import _binding as B
from .alphabet import Alphabet, verify_alphabet_coverage
from .constants import (
    DEFAULT_ALPHA,
    DEFAULT_BEAM_WIDTH,
    DEFAULT_BETA,
    DEFAULT_HOTWORD_WEIGHT,
    DEFAULT_MIN_TOKEN_LOGP,
    DEFAULT_PRUNE_BEAMS,
    DEFAULT_PRUNE_LOGP,
    DEFAULT_SCORE_LM_BOUNDARY,
    DEFAULT_UNK_LOGP_OFFSET,
    LOG_BASE_CHANGE_FACTOR,
)
from .language_model import (
    AbstractLanguageModel,
    AbstractLMState,
    HotwordScorer,
    KenlmState,
    LanguageModel,
    MAX_LANGUAGE_MODELS,
    MultiLanguageModel,
    MultiLanguageModelState,
    NgramModel,
    NgramState,
    _default_device,
    load_unigram_set_from_arpa,
)

logger = logging.getLogger(__name__)

Frames = Tuple[int, int]
WordFrames = Tuple[str, Frames]
# type aliases callers of the reference import from here (decoder.py:121-126, 142-143)
LMScoreCacheKey = Tuple[str, bool]
LMScoreCacheValue = Tuple[float, float, AbstractLMState]
LMScoreCache = Dict[LMScoreCacheKey, LMScoreCacheValue]
FloatVar = TypeVar("FloatVar", bound=np.floating)
Shape = TypeVar("Shape")


@dataclasses.dataclass(frozen=True)
class Beam:
    """decoder.py:69-92 (field order is API)."""

    text: str
    next_word: str
    partial_word: str
    last_char: Optional[str]
    text_frames: List[Frames]
    partial_frames: Frames
    logit_score: float

    @classmethod
    def from_lm_beam(cls, lm_beam: "LMBeam") -> "Beam":
        """The beam without its language-model score (decoder.py:81-92)."""
        return Beam(*(getattr(lm_beam, f.name) for f in dataclasses.fields(Beam)))


@dataclasses.dataclass(frozen=True)
class LMBeam(Beam):
    lm_score: float


@dataclasses.dataclass(frozen=True)
class TokenLMBeam(LMBeam):
    """An LMBeam with the frames of its tokens (partial_decode_beams(..., token_frames=True)), as TokenOutputBeam lists
    them, from the START of the stream: the tokens of the words of ``text_frames`` (words closed by ``force_next_word``
    included), then those of the still open ``partial_word`` -- the last of which ends at ``partial_frames[1]``. Frames are
    absolute, in the numbering of ``text_frames`` / ``partial_frames``."""

    token_frames: List[Tuple[str, Frames]]


@dataclasses.dataclass(frozen=True)
class ConfidenceLMBeam(TokenLMBeam):
    """A TokenLMBeam with confidences (partial_decode_beams(..., confidence="mean" | "min" | "max")), as
    ConfidenceOutputBeam defines them. ``token_logp`` is parallel to ``token_frames`` -- a token that runs across a chunk
    boundary, or lies wholly in an earlier chunk, is folded over all of its frames, and its value is the float64
    decode_beams(confidence=...) gives for the same frames. ``word_logp`` is parallel to ``text_frames``: closed words only,
    the smallest ``token_logp`` among the word's tokens."""

    token_logp: List[float]
    word_logp: List[float]


@dataclasses.dataclass(frozen=True)
class OutputBeam:
    """decoder.py:102-118."""

    text: str
    last_lm_state: Optional[AbstractLMState]
    text_frames: List[WordFrames]
    logit_score: float
    lm_score: float

    def get_mp_safe_beam(self) -> "OutputBeam":
        """A copy that pickles: the LM state is swapped for its process-independent form (decoder.py:112-118)."""
        state = self.last_lm_state
        return dataclasses.replace(self, last_lm_state=state.get_mp_safe_state() if state is not None else None)


@dataclasses.dataclass(frozen=True)
class TokenOutputBeam(OutputBeam):
    """An OutputBeam with the frames of its tokens (decode_beams(..., token_frames=True)): every non-blank emission on the
    beam's path except the space label of a character alphabet, in order, as (label, (start, end)). ``label`` is the
    alphabet label, ``start`` the frame at which the beam took it after a blank or another label, ``end`` 1 + the last
    frame of the run of that label which follows. Each word of ``text_frames`` spans a run of consecutive tokens."""

    token_frames: List[Tuple[str, Frames]]


@dataclasses.dataclass(frozen=True)
class ConfidenceOutputBeam(TokenOutputBeam):
    """A TokenOutputBeam with confidences (decode_beams(..., confidence="mean" | "min" | "max")), as natural-log
    probabilities (<= 0; ``exp()`` gives the [0, 1] form). ``token_logp`` is parallel to ``token_frames``: the fold, over the
    frames ``start .. end - 1`` of the token, of the log-probability the acoustic model gave the token's label at that
    frame (the clipped log-softmax the token prune looks at); "mean" is the arithmetic mean, the log of the geometric mean
    of the probabilities. ``word_logp`` is parallel to ``text_frames``: the smallest ``token_logp`` among the word's tokens."""

    token_logp: List[float]
    word_logp: List[float]

ALIGN_MAX_LABELS = 2047  # ALIGN_MAX_LABELS of csrc/ctc_align.h: 2 L + 1 states, two fp64 score columns in a workgroup's LDS
ALIGN_LONG_MAX_LABELS = 1048575  # ALIGN_LONG_MAX_LABELS of csrc/ctc_align.h: 2 L + 1 states below 2^21 (align_long)
ALIGN_BP_BUDGET = 1 << 30  # bytes of back-pointer tables one ctc_viterbi launch holds by default ("Forced alignment")


@dataclasses.dataclass(frozen=True)
class AlignedText:
    """Where a known transcript lies in the audio (BeamSearchDecoderCTC.align / align_batch): the best CTC path through
    blank / label / blank / ... for the target. ``path`` is the label id taken at each frame (int32 ``[T]``, the blank's id
    for blanks), ``score`` the sum of the clipped log-probabilities along it. ``token_frames`` and ``text_frames`` are those
    of TokenOutputBeam / OutputBeam (end exclusive; the space label of a character alphabet is no token); with
    ``confidence=...`` ``token_logp`` and ``word_logp`` are those of ConfidenceOutputBeam, folded over the token's own frames
    of ``path``, else None."""

    text: str
    path: np.ndarray
    score: float
    token_frames: List[Tuple[str, Frames]]
    text_frames: List[WordFrames]
    token_logp: Optional[List[float]] = None
    word_logp: Optional[List[float]] = None


@dataclasses.dataclass(frozen=True)
class GappedAlignment:
    """Where a transcript that does not cover all of the audio lies in it (BeamSearchDecoderCTC.align_gaps /
    align_gaps_batch; DESIGN.md, "Alignment with gaps"): the best CTC path for a target in which a gap stands wherever
    something was not transcribed. ``text`` is the normalised text with the marker where a gap stands, ``tokens`` the label
    ids with -1 for each gap (adjacent gaps merged). ``path`` is the label id taken at each frame (int32 ``[T]``, the blank's
    id for blanks, -1 on the frames a gap took), ``score`` the sum of the clipped log-probabilities along it, a gap frame
    counting the best any label or the blank has in that frame. ``token_frames``, ``text_frames``, ``token_logp`` and
    ``word_logp`` are AlignedText's: gaps are neither tokens nor words. ``gaps`` holds, per gap in target order, its frames
    ``(start, end)`` (end exclusive; everything between the label before and the label after, so ``start == end`` for an empty
    gap) and ``gap_logp`` the sum of the best log-probability of each of those frames."""

    text: str
    tokens: List[int]
    path: np.ndarray
    score: float
    token_frames: List[Tuple[str, Frames]]
    text_frames: List[WordFrames]
    gaps: List[Frames]
    gap_logp: List[float]
    token_logp: Optional[List[float]] = None
    word_logp: Optional[List[float]] = None


@dataclasses.dataclass(frozen=True, eq=False)
class PrefixScores:
    """How probable it is that the transcript starts with a prefix, and with the prefix followed by each label
    (BeamSearchDecoderCTC.prefix_scores / prefix_scores_batch; DESIGN.md, "Prefix scores"). ``tokens`` are the prefix' label
    ids and ``text`` its normalised text -- with one trailing space where the prefix ends on the space label of a character
    alphabet. ``logp_end`` is the CTC forward score of the prefix as the whole transcript: the float score / score_batch
    returns for it. ``next_logp`` (float64 ``[V]``) holds for every label c the natural log of the mass of all alignments
    whose labels start with ``tokens + [c]`` -- for normalised rows the probability that the transcript starts so --,
    ``-inf`` for the blank and wherever no frame is left for c. For host input it is a numpy array, for device tensors a
    torch tensor on the same device: a view of the call's one ``[prefixes, V]`` allocation."""

    text: str
    tokens: List[int]
    logp_end: float
    next_logp: Any


@dataclasses.dataclass(frozen=True, eq=False)
class SessionPrefix:
    """A live prefix of a PrefixSession: ``id`` is what extend and release take, ``utt`` the utterance it belongs to, and
    ``text``, ``tokens``, ``logp_end`` and ``next_logp`` are PrefixScores' -- the same bits prefix_scores_batch gives for
    ``tokens`` on the session's input. For device input ``next_logp`` is a view of the step's ``[n, V]`` tensor."""

    id: int
    utt: int
    text: str
    tokens: List[int]
    logp_end: float
    next_logp: Any


class PrefixSession:
    """Prefix scores for a decoding loop (BeamSearchDecoderCTC.prefix_session; DESIGN.md, "Prefix sessions"): the session
    keeps every live prefix' end states on the device, so that ``extend`` forms a child -- a live prefix followed by one
    label -- in O(T) (kernel ctc_prefix_advance) instead of a forward pass from label 0, and row_lse and the classification
    run once, when the session opens. ``roots[u]`` is the empty prefix of utterance u. A context manager; ``close()`` frees
    the device memory."""

    def __init__(self, decoder: "BeamSearchDecoderCTC", logits_list: Any, capacity: Optional[int] = None):
        if isinstance(logits_list, (_ResidentBeams, _DeviceStreams)) or (
                isinstance(logits_list, (list, tuple)) and any(isinstance(x, (_ResidentBeams, _DeviceStreams)) for x in logits_list)):
            raise NotImplementedError("a prefix session reads an utterance's matrix at every step; the frames a stream has consumed are not kept")
        if getattr(logits_list, "ndim", 0) != 3:
            logits_list = list(logits_list)
        self._decoder, self._lib = decoder, decoder._lib
        self._handle = None
        n = len(logits_list)
        self._n_labels = len(decoder._labels_list)
        if capacity is None:
            capacity = 64 * n
        if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or capacity < n:
            raise ValueError("prefix_session: capacity must be an int of at least one slot per utterance (%d), not %r" % (n, capacity))
        self.capacity = int(capacity)
        self.last_next = None
        self.last_timing_ms, self.last_launches = (0.0, 0.0, 0.0), (0, 0, 0, 0)
        self._nodes: Dict[int, SessionPrefix] = {}
        self._space = None if decoder._is_bpe else decoder._vocab2idx.get(" ")
        with decoder._call_lock:
            batch, frames, ptrs, c_utts = decoder._stage_transcript_call(logits_list)
            self._batch = batch  # (device tensors are read in place by every extend: they live as long as the session)
            self._is_device = bool(batch.is_device)
            buf, next_dev, next_host = self._room(n)
            ids, end = np.zeros(max(n, 1), dtype=np.int64), np.zeros(max(n, 1), dtype=np.float64)
            handle = C.c_void_p()
            lib = self._lib
            lib.check(lib.dll.ctcdec_prefix_session_open(
                decoder._handle, *c_utts, n,
                batch.dtype, int(batch.is_device), self.capacity, next_dev, B.off_ptr(ids), end.ctypes.data_as(C.POINTER(C.c_double)),
                next_host, C.byref(handle)))
            self._handle = handle
            self._take_timing()
        if not self._is_device:
            self._batch = None  # (host matrices were staged into the session's own memory)
        self.roots: List[SessionPrefix] = self._nodes_of(ids[:n], list(range(n)), [[] for _ in range(n)], end[:n], buf)

    def _room(self, n: int):
        """-> (block, device pointer or None, host pointer or None): the step's [n, V] float64 block, which the kernels fill in
        place for device input."""
        if self._is_device:
            import torch

            buf = torch.empty((n, self._n_labels), dtype=torch.float64, device=self._batch.keep[0].device if self._batch.keep else "cuda")
            return buf, (C.c_void_p(buf.data_ptr()) if n else None), None
        buf = np.empty((n, self._n_labels), dtype=np.float64)
        return buf, None, C.c_void_p(buf.ctypes.data)

    def _take_timing(self) -> None:
        ms, launches = (C.c_double * 3)(), (C.c_int32 * 4)()
        self._lib.dll.ctcdec_prefix_session_timing(self._handle, ms, launches)
        # [ctc_prefix_advance, ctc_prefix_extend with its finish and fill (HIP events), whole native call]; launches of
        # (ctc_prefix_advance, ctc_prefix_extend / finish / fill, row_lse, the forward kernels)
        self.last_timing_ms = tuple(float(v) for v in ms)
        self.last_launches = tuple(int(v) for v in launches)

    def _nodes_of(self, ids, utts, tokens, end, buf) -> List[SessionPrefix]:
        if self._is_device:
            self.last_next = buf
        rows = buf.unbind(0) if self._is_device else list(buf)
        out = []
        for k, (i, u, toks) in enumerate(zip(ids.tolist(), utts, tokens)):
            text = self._decoder._words_of_target(toks)[0] + (" " if toks and toks[-1] == self._space else "")
            node = SessionPrefix(i, u, text, toks, float(end[k]), rows[k])
            self._nodes[i] = node
            out.append(node)
        return out

    def _open_handle(self):
        if self._handle is None:
            raise ValueError("the prefix session is closed")
        return self._handle

    def _live(self, what: str, i: Any) -> SessionPrefix:
        node = self._nodes.get(i) if isinstance(i, (int, np.integer)) and not isinstance(i, bool) else None
        if node is None:
            raise ValueError("%s: %r is not the id of a live prefix of this session" % (what, i))
        return node

    def __len__(self) -> int:
        return len(self._nodes)

    def extend(self, parents: Sequence[int], labels: Optional[Sequence[int]] = None,
               texts: Optional[Sequence[str]] = None) -> List[SessionPrefix]:
        """Child k is the live prefix ``parents[k]`` followed by ``labels[k]`` (or, character alphabets, by the single
        character ``texts[k]``): one ctc_prefix_advance launch for all of them, then ctc_prefix_extend as in
        prefix_scores_batch. A parent may be given any number of times. A ValueError -- a dead or foreign id, the blank, a
        label outside the alphabet, more children than free slots, a child of more than 2047 labels -- leaves the session
        as it was."""
        handle = self._open_handle()
        dec = self._decoder
        if (labels is None) == (texts is None):
            raise ValueError("extend: give exactly one of labels and texts")
        parents = list(parents)
        if texts is not None:
            if dec._is_bpe:
                raise ValueError("a text has many segmentations under a BPE alphabet: give the labels")
            labels = []
            for k, t in enumerate(texts):
                if not isinstance(t, str) or len(t) != 1 or t not in dec._vocab2idx:
                    raise ValueError("extend: texts[%d] is %r: not a single character of the alphabet" % (k, t))
                labels.append(dec._vocab2idx[t])
        labels = list(labels)
        if len(labels) != len(parents):
            raise ValueError("extend: %d labels for %d parents" % (len(labels), len(parents)))
        blank = dec._vocab2idx[""]
        nodes = [self._live("extend", p) for p in parents]
        for k, c in enumerate(labels):
            if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 0 <= int(c) < self._n_labels or int(c) == blank:
                raise ValueError("extend: labels[%d] is %r: not a label id in [0, %d) other than the blank (%d)" % (k, c, self._n_labels, blank))
            if len(nodes[k].tokens) + 1 > ALIGN_MAX_LABELS:
                raise ValueError("extend: child %d has %d labels, above the limit of %d labels per prefix" % (k, len(nodes[k].tokens) + 1, ALIGN_MAX_LABELS))
        n = len(parents)
        if len(self._nodes) + n > self.capacity:
            raise ValueError("extend: %d children, but %d of the session's %d slots are free: release prefixes, or open the session "
                             "with a larger capacity" % (n, self.capacity - len(self._nodes), self.capacity))
        if n == 0:
            return []
        with dec._call_lock:
            buf, next_dev, next_host = self._room(n)
            par = np.ascontiguousarray(parents, dtype=np.int64)
            lab = np.ascontiguousarray([int(c) for c in labels], dtype=np.int32)
            ids, end = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.float64)
            self._lib.check(self._lib.dll.ctcdec_prefix_session_extend(
                handle, B.off_ptr(par), lab.ctypes.data_as(C.POINTER(C.c_int32)), n, next_dev, B.off_ptr(ids),
                end.ctypes.data_as(C.POINTER(C.c_double)), next_host))
            self._take_timing()
        return self._nodes_of(ids, [p.utt for p in nodes], [p.tokens + [int(c)] for p, c in zip(nodes, labels)], end, buf)

    def release(self, ids: Sequence[int]) -> None:
        """The prefixes' slots become free for later children; their ids are dead from here on. The empty prefixes stay."""
        handle = self._open_handle()
        ids = list(ids)
        nodes = [self._live("release", i) for i in ids]
        for node in nodes:
            if not node.tokens:
                raise ValueError("release: %d is the empty prefix of utterance %d, which lives as long as the session" % (node.id, node.utt))
        if len(set(ids)) != len(ids):
            raise ValueError("release: an id is given twice")
        if not ids:
            return
        arr = np.ascontiguousarray(ids, dtype=np.int64)
        with self._decoder._call_lock:
            self._lib.check(self._lib.dll.ctcdec_prefix_session_release(handle, B.off_ptr(arr), len(ids)))
        for i in ids:
            del self._nodes[i]

    def close(self) -> None:
        if self._handle is not None:
            with self._decoder._call_lock:
                self._lib.dll.ctcdec_prefix_session_close(self._handle)
            self._handle = None
            self._nodes.clear()
            self._batch = None

    def __enter__(self) -> "PrefixSession":
        self._open_handle()
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 (interpreter shutdown)
            pass


@dataclasses.dataclass(frozen=True)
class ScoredText:
    """How probable a transcript is, given the audio (BeamSearchDecoderCTC.score / score_batch): ``logp`` is the CTC forward
    score of the label ids ``tokens`` -- the natural log of the sum, over all their alignments, of the product of the frames'
    clipped probabilities -- and ``-inf`` where no alignment exists. ``text`` is the normalised text, formed the way
    AlignedText.text is. ``lm_logp`` (``with_lm=True``, else None) is what the beam search adds for a finished beam with this
    text and no hot words; ``total`` is ``logp + (lm_logp or 0.0)``."""

    text: str
    tokens: List[int]
    logp: float
    lm_logp: Optional[float] = None
    total: float = 0.0


@dataclasses.dataclass(frozen=True, eq=False)
class TranscriptPosteriors:
    """Where, under ALL alignments of a known transcript, each frame lies (BeamSearchDecoderCTC.posteriors /
    posteriors_batch): the CTC forward-backward. ``text`` and ``tokens`` are ScoredText's. ``logp`` is the CTC forward score,
    the float score / score_batch returns for the same input; ``logp_backward`` is the same quantity read off frame 0 of the
    backward pass, a self-check. ``gamma`` (float64 ``[T, 2 L + 1]``, None with ``dense=False``) is the probability that
    frame t is in state s of blank / label 0 / blank / ... / label L - 1 / blank: as computed, so a value may exceed 1 by
    rounding, and exactly 0.0 for a state no alignment can be in at that frame. ``occupancy[k]`` is the expected number of
    frames of token k (the sum over t of ``gamma[t, 2 k + 1]``) and ``centre[k]`` its expected frame; both are summed on the
    device and have the same bits with and without ``dense``."""

    text: str
    tokens: List[int]
    logp: float
    logp_backward: float
    gamma: Optional[np.ndarray]
    occupancy: np.ndarray
    centre: np.ndarray

    @property
    def token_post(self) -> Optional[np.ndarray]:
        """``[T, L]``: the posterior of each token at each frame."""
        return None if self.gamma is None else self.gamma[:, 1::2]

    @property
    def blank_post(self) -> Optional[np.ndarray]:
        """``[T]``: the posterior of a blank, whichever one, at each frame."""
        return None if self.gamma is None else self.gamma[:, 0::2].sum(axis=1)


@dataclasses.dataclass(frozen=True, eq=False)
class TranscriptGradient:
    """What the likelihood of a known transcript asks of each entry of the utterance's matrix (BeamSearchDecoderCTC.gradient /
    gradient_batch): ``text`` and ``tokens`` are ScoredText's, ``logp`` is the CTC forward score, the float score /
    score_batch returns for the same input, and ``grad`` (``[T, V]``) is its derivative with respect to the input as it was
    given -- logits: ``G' - softmax * M`` ("Transcript gradient"; ``G - softmax`` where nothing is clipped);
    probabilities: ``G / p`` -- with derivative 0 wherever the library's clip holds the entry. The sign is logp's: a loss
    negates it. ``grad`` is float64 for float64 input and float32 for float32 / float16 / bfloat16 input (computed in float64,
    rounded once): a numpy array for host input, a torch tensor on the input's device for device tensors."""

    text: str
    tokens: List[int]
    logp: float
    grad: Any


@dataclasses.dataclass(frozen=True)
class PhraseHit:
    """One occurrence of a phrase (BeamSearchDecoderCTC.find / find_batch): the frames ``[start, end)`` -- the first is a frame
    of the phrase's first label, the last a frame of its last label -- and ``logp``, the sum of the clipped log-probabilities
    along the best CTC path of the phrase through exactly those frames."""

    start: int
    end: int
    logp: float

    @property
    def frames(self) -> int:
        return self.end - self.start

    @property
    def mean_logp(self) -> float:
        return self.logp / (self.end - self.start)


@dataclasses.dataclass(frozen=True, eq=False)
class PhraseSearch:
    """Where a phrase occurs in an utterance (BeamSearchDecoderCTC.find / find_batch): ``text`` and ``tokens`` are
    ScoredText's; ``hits`` are the occurrences taken, best first, pairwise disjoint -- none when the utterance has fewer
    frames than the phrase has labels plus adjacent equal labels. With ``trace=True``, ``end_logp[t]`` (float64) is the score
    of the best occurrence whose last label sits on frame ``t`` and ``end_start[t]`` (int32) its first frame, ``-inf`` / ``-1``
    where none ends; else both are None."""

    text: str
    tokens: List[int]
    hits: List[PhraseHit]
    end_logp: Optional[np.ndarray] = None
    end_start: Optional[np.ndarray] = None


POSTERIORS_TABLE_BUDGET = 4 << 30  # bytes of tables one ctc_posteriors launch holds by default ("Frame posteriors")
FORWARD_KERNELS = {"wave": 1, "group": 2}  # ctcdec_score_batch's `kernel` from CTCDEC_FORWARD_KERNEL (unset: the library chooses)
FIND_KERNELS = {"wave": 1, "group": 2}  # ctcdec_find_batch's `kernel` from CTCDEC_FIND_KERNEL (unset: the library chooses)
FIND_MAX_HITS = 64  # FIND_MAX_HITS of csrc/ctc_align.h: a wavefront keeps the windows taken so far one to a lane
CONFIDENCE_FOLDS = {"mean": 2, "min": 3, "max": 4}  # ctcdec_params.token_frames: CTCDEC_TOKEN_LOGP_MEAN / _MIN / _MAX


def _forced_kernel(env_name: str, kernels: Dict[str, int]) -> int:
    """A native call's `kernel` argument from the environment variable that forces one (unset: 0, the library chooses)"""
    name = os.environ.get(env_name, "")
    if name and name not in kernels:
        raise ValueError("%s must be wave or group, not %r" % (env_name, name))
    return kernels.get(name, 0)


def _confidence_fold(confidence: Optional[str]) -> int:
    """The native fold of a ``confidence`` argument (0: none asked for)."""
    if confidence is None:
        return 0
    if not isinstance(confidence, str) or confidence not in CONFIDENCE_FOLDS:
        raise ValueError("confidence must be None, 'mean', 'min' or 'max', not %r" % (confidence,))
    return CONFIDENCE_FOLDS[confidence]


def _word_logps(text_frames: Sequence[WordFrames], token_frames: Sequence[Tuple[str, Frames]],
                token_logp: Sequence[float]) -> List[float]:
    """Per word the smallest token_logp of its run of tokens: those with ``ws <= start`` and ``end <= we``."""
    out, k, n = [], 0, len(token_frames)
    for _, (ws, we) in text_frames:
        while k < n and token_frames[k][1][0] < ws:
            k += 1
        lo = k
        while k < n and token_frames[k][1][1] <= we:
            k += 1
        if k == lo:
            raise RuntimeError("a word of text_frames spans no token of token_frames")
        out.append(min(token_logp[lo:k]))
    return out


class TokenFrames:
    """The token frames of a decode_batch(..., token_frames=True) call as arrays: utterance i's tokens are
    ``[offsets[i], offsets[i + 1])`` of ``label`` (alphabet index), ``start`` and ``end`` (int32); ``offsets`` is int64
    ``[B + 1]``. ``of(i)`` lists them as TokenOutputBeam.token_frames does. ``logp`` is None, or after
    decode_batch(..., confidence=...) the tokens' confidences as a float64 array aligned with ``label``
    (ConfidenceOutputBeam.token_logp; ``logp_of(i)`` lists utterance i's)."""

    __slots__ = ("label", "start", "end", "offsets", "labels", "logp")

    def __init__(self, label: np.ndarray, start: np.ndarray, end: np.ndarray, offsets: np.ndarray, labels: Sequence[str],
                 logp: Optional[np.ndarray] = None):
        self.label, self.start, self.end, self.offsets = label, start, end, offsets
        self.labels = list(labels)
        self.logp = logp

    def __len__(self) -> int:
        return len(self.offsets) - 1

    def of(self, i: int) -> List[Tuple[str, Frames]]:
        lo, hi = int(self.offsets[i]), int(self.offsets[i + 1])
        labels = self.labels
        return [(labels[c], (s, e)) for c, s, e in zip(self.label[lo:hi].tolist(), self.start[lo:hi].tolist(),
                                                        self.end[lo:hi].tolist())]

    def logp_of(self, i: int) -> List[float]:
        if self.logp is None:
            raise ValueError("these token frames were decoded without confidence=...")
        return self.logp[int(self.offsets[i]):int(self.offsets[i + 1])].tolist()

    @classmethod
    def join(cls, parts: Sequence["TokenFrames"], labels: Sequence[str]) -> "TokenFrames":
        """The parts of consecutive slices of a batch as one (offsets rebased)."""
        offs = [np.zeros(1, dtype=np.int64)]
        base = 0
        for t in parts:
            offs.append(t.offsets[1:] + base)
            base += int(t.offsets[-1])
        cat = lambda name: np.concatenate([getattr(t, name) for t in parts]) if parts else np.zeros(0, np.int32)  # noqa: E731
        logp = None
        if parts and all(t.logp is not None for t in parts):
            logp = np.concatenate([t.logp for t in parts])
        return cls(cat("label"), cat("start"), cat("end"), np.concatenate(offs), labels, logp)

    def __reduce__(self):
        return TokenFrames, (self.label, self.start, self.end, self.offsets, self.labels, self.logp)


class GreedyFrames(TokenFrames):
    """The token frames of a decode_greedy_batch(..., token_frames=True) call: TokenFrames (the space label of a character
    alphabet is no token) and ``score``, after decode_greedy_batch(..., confidence=...) a float64 ``[B]`` array -- per utterance
    the sum, over all its frames, of the clipped log-probability of the frame's most probable label (GreedyText.score) --,
    else None."""

    __slots__ = ("score",)

    def __init__(self, label: np.ndarray, start: np.ndarray, end: np.ndarray, offsets: np.ndarray, labels: Sequence[str],
                 logp: Optional[np.ndarray] = None, score: Optional[np.ndarray] = None):
        super().__init__(label, start, end, offsets, labels, logp)
        self.score = score

    @classmethod
    def join(cls, parts: Sequence["GreedyFrames"], labels: Sequence[str]) -> "GreedyFrames":
        """The parts of consecutive slices of a batch as one (offsets rebased)."""
        tf = TokenFrames.join(parts, labels)
        score = None
        if parts and all(t.score is not None for t in parts):
            score = np.concatenate([t.score for t in parts])
        return cls(tf.label, tf.start, tf.end, tf.offsets, labels, tf.logp, score)

    def __reduce__(self):
        return GreedyFrames, (self.label, self.start, self.end, self.offsets, self.labels, self.logp, self.score)


@dataclasses.dataclass(frozen=True)
class GreedyText:
    """The best path over all texts (BeamSearchDecoderCTC.decode_greedy; DESIGN.md, "Greedy decode"): every frame takes its
    most probable label, runs of a label are one token, blanks separate tokens. ``tokens`` are the tokens' label ids -- the
    space label of a character alphabet among them: align(logits, tokens=tokens) is the same path --; ``text``,
    ``token_frames``, ``text_frames``, ``token_logp`` and ``word_logp`` are AlignedText's, for those ids. ``score`` (with
    ``confidence=...``, like ``token_logp`` and ``word_logp``; else None) is the sum over ALL frames of the clipped
    log-probability of the frame's label: what align and align_gaps give for this path, and the upper bound of every
    alignment of the utterance."""

    text: str
    tokens: List[int]
    token_frames: List[Tuple[str, Frames]]
    text_frames: List[WordFrames]
    token_logp: Optional[List[float]] = None
    word_logp: Optional[List[float]] = None
    score: Optional[float] = None


_LM_BEAM_FIELDS = dataclasses.fields(LMBeam)
NULL_FRAMES: Frames = (-1, -1)
EMPTY_START_BEAM = Beam("", "", "", None, [], NULL_FRAMES, 0.0)


def _same_lm_state(a: Any, b: Any) -> bool:
    """Equality of two language-model states by value (one model's, or one per model of a MultiLanguageModel)."""
    if type(a) is not type(b):
        return False
    if hasattr(a, "states"):
        return len(a.states) == len(b.states) and all(_same_lm_state(x, y) for x, y in zip(a.states, b.states))
    return getattr(a, "state", a) == getattr(b, "state", b)


def _is_device_tensor(x: Any) -> bool:
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda")


_CTC_LOSS_FUNCTION = None


def _ctc_loss_function():
    """The torch.autograd.Function behind BeamSearchDecoderCTC.ctc_loss (made on first use: the shell runs without torch)."""
    global _CTC_LOSS_FUNCTION
    if _CTC_LOSS_FUNCTION is not None:
        return _CTC_LOSS_FUNCTION
    import torch

    class CtcLoss(torch.autograd.Function):
        @staticmethod
        def forward(ctx, decoder, texts, tokens, reduction, cube, *xs):
            res, buf, _keep = decoder._gradient_batch(xs[0] if cube else list(xs), texts, tokens, True, 0)
            ctx.cube, ctx.reduction = cube, reduction
            ctx.dtypes = [x.dtype for x in xs]
            # one native call serves both passes: the gradient rows stay on the device until backward
            ctx.grads = [buf.view(xs[0].shape)] if cube and buf is not None else [r.grad for r in res]
            loss = -torch.tensor([r.logp for r in res], dtype=torch.float64, device=xs[0].device)
            return loss.sum() if reduction == "sum" else loss

        @staticmethod
        def backward(ctx, upstream):
            up = upstream.to(torch.float64)
            if ctx.cube:
                scale = up if ctx.reduction == "sum" else up.view(-1, 1, 1)
                grads = [(ctx.grads[0] * -scale).to(ctx.dtypes[0])]
            else:
                grads = [(g * -(up if ctx.reduction == "sum" else up[u])).to(d) for u, (g, d) in enumerate(zip(ctx.grads, ctx.dtypes))]
            return (None, None, None, None, None) + tuple(grads)

    _CTC_LOSS_FUNCTION = CtcLoss
    return CtcLoss


def _is_per_utt_hotwords(hotwords: Any) -> bool:
    """hotwords of decode_batch / decode_beams_batch: None or an iterable of str is one list shared by the whole batch; a
    list or tuple whose entries are None or iterables of str holds one list per utterance. Mixing the two is refused."""
    if not isinstance(hotwords, (list, tuple)) or len(hotwords) == 0:
        return False
    n_str = sum(1 for h in hotwords if isinstance(h, str))
    if n_str == len(hotwords):
        return False
    if n_str > 0:
        raise TypeError("hotwords: either one list of str shared by the batch, or one entry (None or a list of str) per "
                        "utterance -- not a mix of str and lists")
    return True


def _per_utt_hot(hotwords: Any, hotword_weight: Any, n: int, normalise: bool = True):
    """-> None when the batch shares one hot-word list and one weight (the call-wide path, unchanged), else
    (sets, utt_set): the distinct (unigrams, weight) pairs and each utterance's index into them (-1: no hot words).
    Each list is normalised as HotwordScorer.build_scorer normalises a shared one (normalise=False: the lists are a
    HotwordScorer's unigrams already)."""
    per_list = _is_per_utt_hotwords(hotwords)
    per_weight = not isinstance(hotword_weight, (int, float, np.number)) and hasattr(hotword_weight, "__len__")
    if per_list and len(hotwords) != n:
        raise ValueError("hotwords holds %d per-utterance entries for %d utterances" % (len(hotwords), n))
    if per_weight and len(hotword_weight) != n:
        raise ValueError("hotword_weight holds %d per-utterance entries for %d utterances" % (len(hotword_weight), n))
    if not per_list and not per_weight:
        return None
    if per_list:
        lists = []
        seen: Dict[Tuple[str, ...], Tuple[str, ...]] = {}  # (a list repeated over the batch is normalised once)
        for h in hotwords:
            if h is not None and (isinstance(h, str) or not isinstance(h, Iterable)):
                raise TypeError("a per-utterance hotwords entry must be None or an iterable of str")
            raw = tuple(h or ())
            words = seen.get(raw)
            if words is None:
                # build_scorer's rule (strip, drop empties, split phrases into unigrams) without building a scorer
                words = seen[raw] = tuple(w for p in raw for w in p.split()) if normalise else raw
            lists.append(words)
    else:
        shared = tuple(HotwordScorer.build_scorer(hotwords).unigrams)
        lists = [shared] * n
    weights = [float(w) for w in hotword_weight] if per_weight else [float(hotword_weight)] * n
    index: Dict[Tuple[Tuple[str, ...], float], int] = {}
    sets: List[Tuple[Tuple[str, ...], float]] = []
    utt_set: List[int] = []
    for words, w in zip(lists, weights):
        if not words:
            utt_set.append(-1)  # (no hot words: the weight plays no part)
            continue
        key = (words, w)
        k = index.get(key)
        if k is None:
            k = index[key] = len(sets)
            sets.append(key)
        utt_set.append(k)
    return sets, utt_set


class _Batch:
    """Logit matrices of one call, normalised to what the C ABI takes (and shape-checked like
    _check_logits_dimension, decoder.py:330-344)."""

    def __init__(self, logits_list: Sequence[Any], n_labels: int):
        self.keep: List[Any] = []  # keeps buffers alive during the call
        self.ptrs: List[int] = []
        self.frames: List[int] = []
        self.is_device = False
        self.device_index: Optional[int] = None  # device of the logits when they are device tensors
        self.dtype = 0
        if getattr(logits_list, "ndim", 0) == 3 and self._from_3d(logits_list, n_labels):
            return
        n_dev = 0
        for x in logits_list:
            shape = x.shape
            if len(shape) != 2:
                raise ValueError("Input logits have %s dimensions, but need 2: (time, vocabulary)" % len(shape))
            if shape[1] != n_labels:
                raise ValueError(
                    "Input logits shape is %s, but vocabulary is size %s. "
                    "Need logits of shape: (time, vocabulary)" % (tuple(shape), n_labels)
                )
            if getattr(x, "is_cuda", False):
                n_dev += 1
        if n_dev not in (0, len(logits_list)):
            raise ValueError("cannot mix host arrays and device tensors in one batch")
        self.is_device = n_dev > 0
        keep, ptrs, frames = self.keep, self.ptrs, self.frames
        if self.is_device:
            import torch

            native = {torch.float32: 0, torch.float64: 1, torch.float16: 2, torch.bfloat16: 3}
            dtypes = {x.dtype for x in logits_list}
            if len(dtypes) == 1 and next(iter(dtypes)) in native:
                target = next(iter(dtypes))  # fp16 / bf16 / fp32 / fp64 tensors are read in place
            else:
                target = torch.float64 if torch.float64 in dtypes or any(not d.is_floating_point for d in dtypes) \
                    else torch.float32
            for x in logits_list:
                t = x if x.dtype == target else x.to(target)
                if not t.is_contiguous():
                    t = t.contiguous()
                keep.append(t)
                ptrs.append(t.data_ptr())
                frames.append(t.shape[0])
            self.dtype = native[target]
            # Our kernels run on their own stream: the producer of the logits AND the dtype / layout conversions
            # enqueued just above (they run asynchronously on torch's stream) must be done before the native call
            # reads them -- so synchronise AFTER the conversions, on the stream of the tensors' own device.
            devs = {x.device for x in logits_list}
            if len(devs) != 1:
                raise ValueError("the logits of one batch must live on one device")
            dev = next(iter(devs))
            self.device_index = dev.index
            torch.cuda.current_stream(dev).synchronize()
        else:
            arrs = [x.detach().cpu().numpy() if _is_device_tensor(x) else np.asarray(x) for x in logits_list]
            # float32 / float16 matrices go over in their own dtype: the reference decides "probabilities or logits?" on
            # the input dtype (decoder.py:760) and computes a float32 matrix's log-softmax in float32 (decoder.py:180-197), and so
            # does the library. Everything else (float64, integers, batches that mix float32 with float64 / integer matrices --
            # those are computed in float64 altogether, a documented deviation of <= 1e-6 for their float32 members) is widened to
            # float64 first. Matrices without frames have no say.
            kinds = {a.dtype for a in arrs if a.shape[0] > 0}
            target, self.dtype = np.float64, 1
            if kinds == {np.dtype(np.float32)}:
                target, self.dtype = np.float32, 0
            elif kinds == {np.dtype(np.float16)}:
                target, self.dtype = np.float16, 2
            elif kinds and kinds <= {np.dtype(np.float32), np.dtype(np.float16)}:
                target, self.dtype = np.float32, 0
            for a in arrs:
                a = np.ascontiguousarray(a, dtype=target)
                keep.append(a)
                ptrs.append(a.ctypes.data if a.size else 0)
                frames.append(int(a.shape[0]))


    def _from_3d(self, batch: Any, n_labels: int) -> bool:
        """A padded [B, T, V] batch straight from the acoustic model: one pointer + strides instead of B
        per-utterance objects.  Returns False when the generic path has to take over."""
        if batch.shape[2] != n_labels:
            raise ValueError(
                "Input logits shape is %s, but vocabulary is size %s. "
                "Need logits of shape: (time, vocabulary)" % (tuple(batch.shape[1:]), n_labels)
            )
        if getattr(batch, "is_cuda", False):
            import torch

            native = {torch.float32: 0, torch.float64: 1, torch.float16: 2, torch.bfloat16: 3}
            if batch.dtype not in native:
                return False
            t = batch if batch.is_contiguous() else batch.contiguous()
            # (after the possible layout copy, on the batch's own device: see the generic path)
            torch.cuda.current_stream(batch.device).synchronize()
            self.device_index = batch.device.index
            base, step = t.data_ptr(), t.stride(0) * t.element_size()
            self.dtype = native[batch.dtype]
            self.is_device = True
        elif isinstance(batch, np.ndarray):
            target, self.dtype = {np.dtype(np.float32): (np.float32, 0), np.dtype(np.float16): (np.float16, 2)}.get(
                batch.dtype, (np.float64, 1))
            t = np.ascontiguousarray(batch, dtype=target)
            base, step = t.ctypes.data, t.strides[0]
        else:
            return False
        n, frames = int(t.shape[0]), int(t.shape[1])
        self.keep.append(t)
        # (numpy, not 2 x B Python ints: at 4096 utterances the lists and their ctypes copies cost ~1 ms per call)
        self.ptrs = (np.uint64(base) + np.arange(n, dtype=np.uint64) * np.uint64(step)) if n else []
        self.frames = np.full(n, frames, dtype=np.int32) if n else []
        return True


def _c_arrays(batch: _Batch):
    """(void*[n], int32[n]) for the C ABI from a batch's pointer / frame lists (numpy arrays are passed as they are)."""
    n = len(batch.ptrs)
    if isinstance(batch.ptrs, np.ndarray):
        batch.keep.append((batch.ptrs, batch.frames))
        return (batch.ptrs.ctypes.data_as(C.POINTER(C.c_void_p)), batch.frames.ctypes.data_as(C.POINTER(C.c_int32)))
    return (C.c_void_p * max(n, 1))(*batch.ptrs), (C.c_int32 * max(n, 1))(*batch.frames)


class _DeviceStreams:
    """n streams advancing together on the device (one ctcdec_stream handle) + what the Python side has to remember to
    turn their beams into LMBeams on demand."""

    def __init__(self, decoder: "BeamSearchDecoderCTC", n: int):
        self.decoder = decoder
        self.lib = decoder._lib
        self.n = n
        self.gen = 0
        self.hot_key: Optional[Tuple[Any, ...]] = None
        self.hot_sets = None  # per-stream hot words of the last chunk (_per_utt_hot), armed again for every read
        self.params: Optional[B.Params] = None
        self.memos: List[Dict[Any, Any]] = []
        self.parents: Optional[List[List[Beam]]] = None  # the caller's beams of the last import
        self.lists: List[Any] = []  # weak references to the lazy lists of the current generation
        # tokens / confidences (ctcdec_params.token_frames of the stream's chunks; a fold is fixed by the first chunk) and, for
        # the fold's frame numbering, where the next chunk of each stream has to begin
        self.token_mode = 0
        self.next_frame: Optional[List[int]] = None
        h = C.c_void_p()
        self.lib.check(self.lib.dll.ctcdec_stream_open(decoder._handle, n, None, C.byref(h)))
        self.handle = h

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            try:
                self.lib.dll.ctcdec_stream_close(h)
            except Exception:  # pragma: no cover
                pass
            self.handle = None

    def alive(self, decoder) -> bool:
        return self.handle is not None and self.decoder is decoder

    # -- the slow way in: beams the caller built or edited (decoder.py:681-728 takes any List[Beam]) -------------
    def import_beams(self, beams_list, cached_lm_scores_list, hot_sets=None) -> None:
        dec = self.decoder
        n_lms = len(dec._members)
        has_lm = n_lms > 0
        vocab2idx = dec._vocab2idx
        pieces: List[bytes] = []
        pos = 0
        total = sum(len(b) for b in beams_list)
        arr = (B.BeamIn * max(total, 1))()
        more = (B.LmState * max(total * (n_lms - 1), 1))() if n_lms > 1 else None  # model 1..'s states per beam
        beam_off = np.zeros(self.n + 1, dtype=np.int64)
        k = 0
        parents = []
        for u in range(self.n):
            beams = list(beams_list[u])
            parents.append(beams)
            for beam in beams:
                text = beam.text if not beam.next_word else (beam.text + " " + beam.next_word if beam.text else beam.next_word)
                text = " ".join(text.split())
                e = arr[k]
                e.logit_score = float(beam.logit_score)
                if has_lm:
                    raw, state = dec._memo_entry(cached_lm_scores_list[u], text)
                    if n_lms > 1:
                        if not isinstance(state, MultiLanguageModelState) or len(state.states) != n_lms:
                            raise AssertionError(
                                f"Wrong input state type found. Expected MultiLanguageModelState of {n_lms}, got {type(state)}")
                        parts = state.states
                        for j in range(1, n_lms):
                            more[k * (n_lms - 1) + j - 1] = parts[j].state.to_c()
                        e.more_states = C.cast(C.byref(more, k * (n_lms - 1) * C.sizeof(B.LmState)), C.POINTER(B.LmState))
                        state = parts[0]
                    if not isinstance(state, KenlmState):
                        raise AssertionError(f"Wrong input state type found. Expected KenlmState, got {type(state)}")
                    e.raw_lm_score = float(raw)
                    e.lm_state = state.state.to_c()
                if beam.last_char is None:
                    e.last_char = -1
                else:
                    if beam.last_char not in vocab2idx:
                        raise ValueError("beam.last_char %r is not a label of this decoder" % (beam.last_char,))
                    e.last_char = vocab2idx[beam.last_char]
                e.partial_start = int(beam.partial_frames[0])
                e.partial_end_frame = int(beam.partial_frames[1])
                tb = text.encode("utf-8")
                pb = beam.partial_word.encode("utf-8")
                e.text_begin, e.text_end = pos, pos + len(tb)
                pos += len(tb)
                e.partial_begin, e.partial_end = pos, pos + len(pb)
                pos += len(pb)
                pieces.append(tb)
                pieces.append(pb)
                k += 1
            beam_off[u + 1] = k
        blob = b"".join(pieces) or b"\0"
        if hot_sets is not None:  # (each stream's words are counted against its own set)
            dec._arm_hot_sets(hot_sets)
        self.lib.check(self.lib.dll.ctcdec_stream_import(self.handle, arr, B.off_ptr(beam_off), blob, pos))
        self.parents = parents

    # -- results ---------------------------------------------------------------------------------------------------
    def retire_lists(self) -> None:
        """The device is about to move on: lists of the current generation that nobody has looked at become unreadable."""
        self.gen += 1
        self.lists = []

    def lazy_lists(self) -> List[List[LMBeam]]:
        import weakref

        out = [_ResidentBeams(self, u, self.gen) for u in range(self.n)]
        self.lists = [weakref.ref(x) for x in out]
        return out

    def fill_current(self) -> None:
        """One native read materialises the beams of every stream (the lazy lists of this generation that are still alive)."""
        dec = self.decoder
        with dec._call_lock:
            res = C.c_void_p()
            if self.hot_sets is not None:
                dec._arm_hot_sets(self.hot_sets)
            self.lib.check(self.lib.dll.ctcdec_stream_read(self.handle, C.byref(self.params), C.byref(res)))
            try:
                got = self.unpack(res)
            finally:
                self.lib.dll.ctcdec_result_free(res)
        for u, ref in enumerate(self.lists):
            lst = ref()
            if lst is not None and not lst._filled:
                list.extend(lst, got[u])
                lst._filled = True

    def peek_best(self) -> None:
        """`beams[0]` on an unread list (a streaming caller showing the transcript so far): one native read with
        n_best = 1 fetches the best beam of every stream; the lists stay unread otherwise."""
        dec = self.decoder
        with dec._call_lock:
            p = B.Params.from_buffer_copy(self.params)
            p.n_best = 1
            res = C.c_void_p()
            if self.hot_sets is not None:
                dec._arm_hot_sets(self.hot_sets)
            self.lib.check(self.lib.dll.ctcdec_stream_read(self.handle, C.byref(p), C.byref(res)))
            try:
                got = self.unpack(res)
            finally:
                self.lib.dll.ctcdec_result_free(res)
        for u, ref in enumerate(self.lists):
            lst = ref()
            if lst is not None and not lst._filled:
                lst._best = got[u][0] if got[u] else None
                lst._peeked = True

    def unpack(self, res) -> List[List[LMBeam]]:
        """The beams of a stream result; with token_frames / confidence as TokenLMBeams / ConfidenceLMBeams."""
        out = self._unpack_plain(res)
        mode = int(self.params.token_frames) if self.params is not None else 0
        if not mode:
            return out
        with_logp = mode > 1
        tf = self.decoder._token_frames(res, sum(len(bs) for bs in out), with_logp)
        k = 0
        for bs in out:
            for i, b in enumerate(bs):
                base = tuple(getattr(b, f.name) for f in _LM_BEAM_FIELDS)
                toks = tf.of(k)
                if with_logp:
                    lps = tf.logp_of(k)
                    words = _word_logps([(None, f) for f in b.text_frames], toks, lps)
                    bs[i] = ConfidenceLMBeam(*base, toks, lps, words)
                else:
                    bs[i] = TokenLMBeam(*base, toks)
                k += 1
        return out

    def _unpack_plain(self, res) -> List[List[LMBeam]]:
        dec = self.decoder
        lib = self.lib
        n = self.n
        n_lms = len(dec._members)
        has_lm = n_lms > 0
        pk = B.Packed()
        lib.check(lib.dll.ctcdec_result_pack(res, C.byref(pk)))
        nb, nw = int(pk.n_beams), int(pk.n_words)
        if nb == 0:
            return [[] for _ in range(n)]
        b_off = np.ctypeslib.as_array(pk.beam_off, shape=(n + 1,))
        if self.parents is None and not os.environ.get("CTCDEC_PY_UNPACK"):
            # the same lists from one C loop (csrc/pytexts.c); the memo entries of new texts are added here
            frames_of = None
            if not os.environ.get("CTCDEC_EAGER_FRAMES"):  # (diagnostics / tests: plain lists of tuples built in C)
                if nw:
                    ws = np.ctypeslib.as_array(pk.word_start, shape=(nw,)).copy()
                    we = np.ctypeslib.as_array(pk.word_end, shape=(nw,)).copy()
                else:
                    ws = we = np.zeros(0, dtype=np.int32)
                frames_of = _lazy_frames_factory(ws, we)
            built = B.lm_beams(LMBeam, n, pk, dec._labels_list, frames_of)
            if built is not None:
                if has_lm:
                    self._note_memo_entries(res, pk, built, b_off, nb, n_lms)
                return built
        t_off = np.ctypeslib.as_array(pk.text_off, shape=(nb + 1,))
        tblob = C.string_at(pk.text_blob, int(t_off[nb])) if t_off[nb] else b""
        p_off = np.ctypeslib.as_array(pk.partial_off, shape=(nb + 1,))
        pblob = C.string_at(pk.partial_blob, int(p_off[nb])) if p_off[nb] else b""
        logit = np.ctypeslib.as_array(pk.logit_score, shape=(nb,))
        lms = np.ctypeslib.as_array(pk.lm_score, shape=(nb,))
        raw = np.ctypeslib.as_array(pk.raw_lm_score, shape=(nb,))
        src = np.ctypeslib.as_array(pk.src_beam, shape=(nb,))
        lch = np.ctypeslib.as_array(pk.last_char, shape=(nb,))
        ps = np.ctypeslib.as_array(pk.partial_start, shape=(nb,))
        pe = np.ctypeslib.as_array(pk.partial_end, shape=(nb,))
        wco = np.ctypeslib.as_array(pk.word_cnt_off, shape=(nb + 1,))
        if nw:
            wstart = np.ctypeslib.as_array(pk.word_start, shape=(nw,))
            wend = np.ctypeslib.as_array(pk.word_end, shape=(nw,))
        out: List[List[LMBeam]] = []
        for u in range(n):
            outs = []
            memo = self.memos[u] if u < len(self.memos) else {}
            for j in range(int(b_off[u]), int(b_off[u + 1])):
                text = tblob[int(t_off[j]) : int(t_off[j + 1])].decode("utf-8")
                partial = pblob[int(p_off[j]) : int(p_off[j + 1])].decode("utf-8")
                new_frames = [(int(wstart[w]), int(wend[w])) for w in range(int(wco[j]), int(wco[j + 1]))]
                if src[j] >= 0 and self.parents is not None:  # decoded below one of the caller's own beams
                    new_frames = list(self.parents[u][int(src[j])].text_frames) + new_frames
                last = None if lch[j] < 0 else dec._idx2vocab[int(lch[j])]
                outs.append(LMBeam(text, "", partial, last, new_frames, (int(ps[j]), int(pe[j])), float(logit[j]), float(lms[j])))
                if has_lm and (text, False) not in memo:
                    memo[(text, False)] = (float(raw[j]), float(raw[j]), self._state_of(res, pk, u, j, j - int(b_off[u]), n_lms))
            out.append(outs)
        return out

    def _note_memo_entries(self, res, pk, built, b_off, nb: int, n_lms: int) -> None:
        """The caller's caches get an entry for every returned text, as the reference's decode leaves them (decoder.py:387-396).
        A cache that get_starting_state() handed out (_LazyMemo) takes ONE note per read and makes the entries when somebody
        looks; a caller's own dict is filled here. The entries' LM-state objects are made on demand from a private copy of the
        read's packed states (several LMs: eagerly, one native call per beam -- rare, short lists)."""
        raws = np.ctypeslib.as_array(pk.raw_lm_score, shape=(nb,)).tolist()
        sz = C.sizeof(B.LmState)
        whole = C.string_at(C.cast(pk.lm_state, C.c_void_p), nb * sz)
        for u in range(self.n):
            memo = self.memos[u] if u < len(self.memos) else {}
            j0 = int(b_off[u])
            beams = built[u]
            # (a stream's entries keep only that stream's slice of the read's packed states and scores alive)
            store = _StateStore(whole[j0 * sz:(j0 + len(beams)) * sz])
            if n_lms == 1 and type(memo) is _LazyMemo:
                memo._note(beams, raws[j0:j0 + len(beams)], store)
                continue
            j = j0
            for beam in beams:
                key = (beam.text, False)
                if key not in memo:
                    if n_lms > 1:
                        memo[key] = (raws[j], raws[j], self._state_of(res, pk, u, j, j - j0, n_lms))
                    else:
                        memo[key] = _MemoEntry.make(raws[j], store, j - j0)
                j += 1

    def _state_of(self, res, pk, u: int, j: int, j_in_stream: int, n_lms: int) -> AbstractLMState:
        state: AbstractLMState = KenlmState(NgramState.from_c(pk.lm_state[j]))
        if n_lms > 1:
            parts = [state]
            for x in range(1, n_lms):
                cst = B.LmState()
                self.lib.check(self.lib.dll.ctcdec_result_lm_state_of(res, u, j_in_stream, x, C.byref(cst)))
                parts.append(KenlmState(NgramState.from_c(cst)))
            state = MultiLanguageModelState(parts)
        return state


class _LazyFrames(list):
    """text_frames of a returned beam -- an LMBeam's (start, end) pairs, an OutputBeam's (word, (start, end)) pairs --, kept as a
    window of the result's two
    int32 arrays until somebody looks (then an ordinary list of tuples, equal to what the reference returns,
    decoder.py:653-667). A stream that has run for a thousand frames carries ~250 words per beam; building their tuples for
    every beam of every stream was most of the time of reading the beams (round 4: 7.8 ms for 64 streams, 11.3 ms with the
    last chunk), and a caller that hands the beams back, shows the best text or looks at one beam's frames never needs them.
    Same caveat as _ResidentBeams for code that reads list storage through the C API without calling a method."""

    __slots__ = ("_src", "_lo", "_hi", "_text")

    def __init__(self, *a) -> None:
        # (an instance made as type(frames)(iterable) -- dataclasses.asdict and copy-like idioms rebuild list fields that way --
        #  is an ordinary, already filled list)
        self._src = None
        self._lo = self._hi = 0
        self._text = None
        list.__init__(self, *a)

    def _fill(self) -> None:
        src = self._src
        if src is not None:
            self._src = None
            ws, we = src
            spans = zip(ws[self._lo:self._hi].tolist(), we[self._lo:self._hi].tolist())
            text = self._text
            if text is None:  # an LMBeam's frames: (start, end) per word
                list.extend(self, spans)
            else:  # an OutputBeam's: (word, (start, end)) (decoder.py:653-667)
                self._text = None
                list.extend(self, zip(text.split(" ") if text else (), spans))

    _touch = _fill

    def __reduce__(self):
        self._fill()
        return (list, (list(list.__iter__(self)),))


def _lazy_frames_factory(word_start, word_end):
    """frames_of(w0, w1) over private copies of a result's word_start / word_end arrays (the result is freed after the read)"""
    src = (word_start, word_end)

    def frames_of(lo, hi):
        f = _LazyFrames()
        f._src = src
        f._lo = lo
        f._hi = hi
        f._text = None
        return f

    return frames_of


def _lazy_word_frames_factory(word_start, word_end):
    """frames_of(text, w0, w1) for OutputBeams: the words of `text` paired with their frames when somebody looks"""
    src = (word_start, word_end)

    def frames_of(text, lo, hi):
        f = _LazyFrames()
        f._src = src
        f._lo = lo
        f._hi = hi
        f._text = text
        return f

    return frames_of


class _StateStore:
    """The packed LM states of one device read (a private copy: the result is freed after the read) and the state objects made
    from them so far."""

    __slots__ = ("_bytes", "_made")

    def __init__(self, state_bytes: bytes):
        self._bytes = state_bytes
        self._made: Dict[int, AbstractLMState] = {}

    def state(self, j: int) -> AbstractLMState:
        st = self._made.get(j)
        if st is None:
            st = KenlmState(NgramState.from_c(B.LmState.from_buffer_copy(self._bytes, j * C.sizeof(B.LmState))))
            self._made[j] = st
        return st


class _MemoEntry(tuple):
    """A memo entry (lm_score + hot-word score, raw lm_score, LM state) of a text a device read returned -- the tuple the
    reference's cache holds (decoder.py:387-396) -- whose STATE object is built from the read's packed states when somebody
    unpacks or indexes the entry (the import path of edited beams does; a caller that only hands its caches back never does).
    Storage: (raw, raw, store, index); every way of looking sees the three-tuple."""

    __slots__ = ()

    @staticmethod
    def make(raw, store: _StateStore, j: int) -> "_MemoEntry":
        return tuple.__new__(_MemoEntry, (raw, raw, store, j))

    def _full(self):
        g = tuple.__getitem__
        return (g(self, 0), g(self, 1), g(self, 2).state(g(self, 3)))

    def __len__(self):
        return 3

    def __getitem__(self, k):
        return self._full()[k]

    def __iter__(self):
        return iter(self._full())

    def __eq__(self, other):
        return self._full() == (other._full() if isinstance(other, _MemoEntry) else other)

    def __ne__(self, other):
        return not self.__eq__(other)

    __hash__ = None  # type: ignore[assignment]

    def __repr__(self):
        return repr(self._full())

    def __reduce__(self):
        return (tuple, (self._full(),))


class _LazyMemo(dict):
    """`cached_lm_scores` as get_starting_state() hands it out (decoder.py:669-679): a dict that remembers what the device reads
    of its stream returned -- one O(1) note per read -- and turns the notes into entries when somebody LOOKS (any dict method;
    the import path of edited beams does). The reference fills this cache as a side effect of decoding; doing that eagerly was
    a tuple, a dict probe and an entry object per returned beam on every read, for a caller that almost never looks.
    A caller's own plain dict is filled eagerly as before."""

    __slots__ = ("_pending",)

    def __init__(self, *a, **k):
        dict.__init__(self, *a, **k)
        self._pending: List[Any] = []

    _MAX_PENDING = 8

    def _note(self, beams, raws, store: _StateStore) -> None:
        # a snapshot of the read's beams (the caller may sort / delete in the list it was handed; entries pair beams with the
        # stream's slice of the read's raw scores and states BY POSITION); a stream that is read
        # every chunk and never looks at its cache settles after a few notes instead of pinning every read it ever made
        self._pending.append((tuple(beams), raws, store))
        if len(self._pending) > self._MAX_PENDING:
            self._settle()

    def _settle(self) -> None:
        pend = self._pending
        if pend:
            self._pending = []
            has, put, make = dict.__contains__, dict.__setitem__, _MemoEntry.make
            for beams, raws, store in pend:
                for k, beam in enumerate(beams):
                    key = (beam.text, False)
                    if not has(self, key):
                        put(self, key, make(raws[k], store, k))

    def __reduce__(self):
        self._settle()
        return (dict, (dict(dict.items(self)),))


def _settling(name):
    def method(self, *a, **k):
        self._settle()
        return getattr(dict, name)(self, *a, **k)

    method.__name__ = name
    return method


for _n in ("__getitem__", "__contains__", "__iter__", "__len__", "__repr__", "__eq__", "__ne__", "get", "keys", "values", "items",
           "copy", "pop", "popitem", "setdefault", "update", "__delitem__", "clear", "__or__", "__ror__", "__ior__", "__reversed__"):
    setattr(_LazyMemo, _n, _settling(_n))
_LazyMemo.__hash__ = None  # type: ignore[assignment]


class _ResidentBeams(list):
    """The LMBeams of one stream after a chunk, still on the device: an ordinary list that fills itself the first time it
    is looked at. Handed back unchanged to partial_decode_beams(_batch) it is never filled at all.
    Caveat: code that reads a list through the C API without calling a method (PySequence_Fast / PyList_GET_SIZE on a
    subclass: the C json encoder, some extension modules) sees the unfilled storage -- pass list(beams) to such code.
    Pickling and copying go through __reduce__ and yield a plain, filled list."""

    def __init__(self, streams: _DeviceStreams, index: int, gen: int):
        super().__init__()
        self._streams = streams
        self._index = index
        self._gen = gen
        self._filled = False
        self._edited = False
        self._peeked = False
        self._best: Optional[LMBeam] = None

    def __getitem__(self, key):
        # the best beam alone is a cheap read (n_best = 1); anything else fills the list
        if not self._filled and type(key) is int and key == 0 and self._gen == self._streams.gen:
            if not self._peeked:
                self._streams.peek_best()
            if self._best is not None:
                return self._best
        self._fill()
        return list.__getitem__(self, key)

    def _current(self) -> bool:
        return not self._edited and self._gen == self._streams.gen

    def __reduce__(self):
        # pickle / copy / multiprocessing: as the plain list of its beams (the device handle stays behind)
        self._fill()
        return (list, (list(list.__iter__(self)),))

    def _fill(self) -> None:
        if self._filled:
            return
        if self._gen != self._streams.gen:
            raise RuntimeError(
                "these beams were handed back to partial_decode_beams and the stream has moved on: read them before the "
                "next call, or keep list(beams) (CTCDEC_RESIDENT_STREAMS=0 returns plain lists every time)")
        self._streams.fill_current()

    def _touch(self) -> None:
        self._fill()
        self._edited = True


def _fill_args(args) -> None:
    # (the list type's own C code reads another lazy list's storage directly: a comparison / concatenation / extend with one
    #  has to fill it first)
    for x in args:
        if isinstance(x, (_LazyFrames, _ResidentBeams)):
            x._fill()


def _reader(name):
    def method(self, *a, **k):
        self._fill()
        _fill_args(a)
        return getattr(list, name)(self, *a, **k)

    method.__name__ = name
    return method


def _writer(name):
    def method(self, *a, **k):
        self._touch()
        _fill_args(a)
        return getattr(list, name)(self, *a, **k)

    method.__name__ = name
    return method


for _n in ("__len__", "__iter__", "__contains__", "__repr__", "__eq__", "__ne__", "__lt__", "__le__", "__gt__",
           "__ge__", "__add__", "__mul__", "__rmul__", "__reversed__", "index", "count", "copy"):
    setattr(_ResidentBeams, _n, _reader(_n))
for _n in ("__setitem__", "__delitem__", "__iadd__", "__imul__", "append", "extend", "insert", "pop", "remove", "clear", "sort",
           "reverse"):
    setattr(_ResidentBeams, _n, _writer(_n))
_ResidentBeams.__hash__ = None  # type: ignore[assignment]


def _radd(self, other):
    # plain_list + lazy: a subclass's reflected method is tried first, which is the only chance to fill before list's C code
    # concatenates the (still empty) storage
    self._fill()
    return list(other) + list(list.__iter__(self))


_ResidentBeams.__radd__ = _radd  # type: ignore[attr-defined]
_LazyFrames.__radd__ = _radd  # type: ignore[attr-defined]
for _n in ("__len__", "__iter__", "__contains__", "__repr__", "__eq__", "__ne__", "__lt__", "__le__", "__gt__", "__ge__", "__add__",
           "__mul__", "__rmul__", "__reversed__", "index", "count", "copy", "__getitem__", "__setitem__", "__delitem__", "__iadd__",
           "__imul__", "append", "extend", "insert", "pop", "remove", "clear", "sort", "reverse"):
    setattr(_LazyFrames, _n, _reader(_n))
_LazyFrames.__hash__ = None  # type: ignore[assignment]


class BeamSearchDecoderCTC:
    # The reference parks the language model in a class-level dict keyed by 16 random bytes so that
    # fork-pool children find it (decoder.py:262-269); the container and its clean-up functions
    # are kept because callers and tests manage memory through them.
    model_container: Dict[bytes, Optional[AbstractLanguageModel]] = {}

    def __init__(self, alphabet: Alphabet, language_model: Optional[AbstractLanguageModel] = None) -> None:
        self._alphabet = alphabet
        self._idx2vocab = {n: c for n, c in enumerate(self._alphabet.labels)}
        self._labels_list = list(self._alphabet.labels)
        self._vocab2idx = {c: n for n, c in enumerate(self._alphabet.labels)}
        self._is_bpe = alphabet.is_bpe
        self._model_key = os.urandom(16)
        BeamSearchDecoderCTC.model_container[self._model_key] = language_model
        members: List[LanguageModel] = []
        if isinstance(language_model, MultiLanguageModel):
            members = language_model.language_models
            if len(members) > MAX_LANGUAGE_MODELS:
                raise NotImplementedError("a MultiLanguageModel of more than %d models" % MAX_LANGUAGE_MODELS)
        elif language_model is not None:
            members = [language_model]
        if not all(isinstance(m, LanguageModel) for m in members):
            raise NotImplementedError(
                "only n-gram LanguageModels (alone or inside a MultiLanguageModel) can be lowered to the "
                "device trie; user-defined AbstractLanguageModel subclasses are not supported "
                "(there is deliberately no CPU fallback)"
            )
        self._members = members
        self._device = _default_device()  # one process per GPU: LOCAL_RANK, or CTCDEC_DEVICE when set
        lib = B.get_library()
        self._lib = lib
        blob, off = B.pack_strings(self._alphabet.labels)
        handle = C.c_void_p()
        lib.check(
            lib.dll.ctcdec_create(blob, B.off_ptr(off), len(self._alphabet.labels), int(self._is_bpe),
                                  self._device, C.byref(handle))
        )
        self._handle = handle
        # the device the library actually bound (one visible GPU per rank under SLURM / HIP_VISIBLE_DEVICES: LOCAL_RANK may
        # exceed the device count and the library falls back to device 0)
        self._device = int(lib.dll.ctcdec_device())
        if len(members) == 1:
            lib.check(lib.dll.ctcdec_lm_share(handle, members[0]._kenlm_model._handle))
        elif len(members) > 1:
            srcs = (C.c_void_p * len(members))(*[m._kenlm_model._handle for m in members])
            lib.check(lib.dll.ctcdec_lm_share_multi(handle, srcs, len(members)))
        self._hot_key: Optional[Tuple[str, ...]] = None
        # a byte no decoded text can contain (texts are made of label characters and spaces): lets decode_batch take its
        # texts as one joined buffer and split it natively
        self._texts_sep: Optional[bytes] = next(
            (c.encode("ascii") for c in ("\n", "\x01", "\x02") if not any(c in lab for lab in self._alphabet.labels)), None)
        # one native call at a time per decoder: hot words / per-model weights are decoder state that a call sets
        # up first (host threads may share a decoder; ctypes releases the GIL while the device works)
        self._call_lock = threading.RLock()
        # diagnostics of the last score / score_batch call (ms: classification, row_lse, forward kernels, native call;
        # hypotheses taken by the wave kernel and by the group kernel)
        self.last_score_timing_ms = (0.0, 0.0, 0.0, 0.0)
        self.last_score_launched = (0, 0)
        # ... and of the last posteriors / posteriors_batch call (ms likewise; kernel launches made; utterances taken by the
        # 256-thread and by the 1024-thread kernel)
        self.last_posteriors_timing_ms = (0.0, 0.0, 0.0, 0.0)
        self.last_posteriors_launches = 0
        self.last_posteriors_launched = (0, 0)
        # ... and of the last gradient / gradient_batch / ctc_loss call (ms: classification, row_lse, ctc_posteriors,
        # ctc_grad_rows, whole native call; launches of both kernels; utterances by ctc_posteriors instantiation)
        self.last_gradient_timing_ms = (0.0, 0.0, 0.0, 0.0, 0.0)
        self.last_gradient_launches = 0
        self.last_gradient_launched = (0, 0)
        # ... and of the last find / find_batch call (ms: classification, row_lse, find kernels, native call; kernel launches
        # made; phrases taken by the wave kernel and by the group kernel)
        self.last_find_timing_ms = (0.0, 0.0, 0.0, 0.0)
        self.last_find_launches = 0
        self.last_find_launched = (0, 0)
        # ... and of the last align_gaps / align_gaps_batch call (ms: classification, row_lse_max, ctc_viterbi_gaps, native
        # call; kernel launches made)
        self.last_align_gaps_timing_ms = (0.0, 0.0, 0.0, 0.0)
        self.last_align_gaps_launches = 0
        # ... and of the last align_long / align_long_batch call (ms: classification, row_lse, ctc_viterbi_long, native call;
        # kernel launches made; (segment_frames, n_segments) of every utterance that was aligned)
        self.last_align_long_timing_ms = (0.0, 0.0, 0.0, 0.0)
        self.last_align_long_launches = 0
        self.last_align_long_plan: List[Tuple[int, int]] = []
        # ... and of the last decode_greedy / decode_greedy_batch call (ms: classification, row_argmax or row_lse_argmax,
        # greedy_collapse, native call; kernel launches made; the part of the row kernel's time that a kernel with a
        # log-sum-exp took: 0 without confidence=...)
        self.last_greedy_timing_ms = (0.0, 0.0, 0.0, 0.0)
        self.last_greedy_launches = 0
        self.last_greedy_lse_ms = 0.0
        # ... and of the last prefix_scores / prefix_scores_batch call (ms: classification, row_lse, forward kernels with end
        # states, ctc_prefix_extend, native call; prefixes taken by the wave and by the group forward kernel; kernel launches
        # of row_lse, of the forward kernels and of ctc_prefix_extend with its finish and fill) and, for device input, the [prefixes, V] tensor every next_logp of that call is a view of
        self.last_prefix_timing_ms = (0.0, 0.0, 0.0, 0.0, 0.0)
        self.last_prefix_launched = (0, 0)
        self.last_prefix_launches = (0, 0, 0)
        self.last_prefix_next = None

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h is not None:
            try:
                self._lib.dll.ctcdec_destroy(h)
            except Exception:  # pragma: no cover
                pass
            self._handle = None

    # -- parameter / model management (decoder.py:292-328) -------------------------------------
    def reset_params(
        self,
        alpha: Optional[float] = None,
        beta: Optional[float] = None,
        unk_score_offset: Optional[float] = None,
        lm_score_boundary: Optional[bool] = None,
    ) -> None:
        """Forward the weights that were given to the language model (decoder.py:292-316); no model, nothing to do."""
        lm = self._language_model
        if lm is None:
            return
        given = {"alpha": alpha, "beta": beta, "unk_score_offset": unk_score_offset, "score_boundary": lm_score_boundary}
        lm.reset_params(**{name: value for name, value in given.items() if value is not None})

    @classmethod
    def clear_class_models(cls) -> None:
        cls.model_container = {}

    def cleanup(self) -> None:
        if self._model_key in BeamSearchDecoderCTC.model_container:
            del BeamSearchDecoderCTC.model_container[self._model_key]

    @property
    def _language_model(self) -> Optional[AbstractLanguageModel]:
        return BeamSearchDecoderCTC.model_container[self._model_key]

    def _check_logits_dimension(self, logits: Any) -> None:
        if len(logits.shape) != 2:
            raise ValueError(
                "Input logits have %s dimensions, but need 2: (time, vocabulary)" % len(logits.shape)
            )
        if logits.shape[-1] != len(self._idx2vocab):
            raise ValueError(
                "Input logits shape is %s, but vocabulary is size %s. "
                "Need logits of shape: (time, vocabulary)" % (tuple(logits.shape), len(self._idx2vocab))
            )

    # -- the one native call everything funnels into --------------------------------------------
    def _set_hotwords(self, hotwords: Optional[Iterable[str]]) -> None:
        unigrams = HotwordScorer.build_scorer(hotwords).unigrams
        key = tuple(unigrams)
        if key == self._hot_key:
            return
        blob, off = B.pack_strings(unigrams)
        self._lib.check(self._lib.dll.ctcdec_set_hotwords(self._handle, blob, B.off_ptr(off), len(unigrams)))
        self._hot_key = key

    def _arm_hot_sets(self, hot) -> None:
        """ctcdec_set_hotword_sets for the next native call: hot = _per_utt_hot(...)'s (sets, utt_set)."""
        sets, utt_set = hot
        words = [w for ws, _ in sets for w in ws]
        blob, off = B.pack_strings(words)
        set_off = np.zeros(len(sets) + 1, dtype=np.int64)
        if sets:
            set_off[1:] = np.cumsum([len(ws) for ws, _ in sets])
        weight = np.array([w for _, w in sets] or [0.0], dtype=np.float64)
        idx = np.array(utt_set or [0], dtype=np.int32)
        self._lib.check(self._lib.dll.ctcdec_set_hotword_sets(
            self._handle, blob, B.off_ptr(off), len(words), B.off_ptr(set_off), len(sets),
            weight.ctypes.data_as(C.POINTER(C.c_double)), idx.ctypes.data_as(C.POINTER(C.c_int32)), len(utt_set)))

    def _resolve_hot(self, hotwords, hotword_weight, n: int):
        """-> (hotwords, hotword_weight, per-utterance sets or None) for a batch call. A batch whose utterances all end up
        with one list and one weight goes the call-wide way (one set, the same bits as a shared list)."""
        hot = _per_utt_hot(hotwords, hotword_weight, n)
        if hot is None:
            return hotwords, hotword_weight, None
        sets, utt_set = hot
        if all(k == utt_set[0] for k in utt_set):
            if utt_set[0] < 0:
                return None, DEFAULT_HOTWORD_WEIGHT, None
            words, w = sets[utt_set[0]]
            return list(words), w, None
        return None, DEFAULT_HOTWORD_WEIGHT, hot

    def _params(self, beam_width, beam_prune_logp, token_min_logp, prune_history, hotword_weight, n_best) -> B.Params:
        lm = self._members[0] if self._members else None  # model 0; the others go through ctcdec_lm_set_params
        with self._call_lock:  # (RLock: the streaming path already holds it; nothing may change the handle mid-call)
            for k, m in enumerate(self._members[1:], start=1):
                self._lib.check(self._lib.dll.ctcdec_lm_set_params(
                    self._handle, k, float(m.alpha), float(m.beta), float(m.unk_score_offset), int(bool(m.score_boundary))))
        p = B.Params()
        p.beam_width = int(beam_width)
        p.prune_history = int(bool(prune_history))
        p.n_best = int(n_best)
        p.want_lm_state = 1
        p.beam_prune_logp = float(beam_prune_logp)
        p.token_min_logp = float(token_min_logp)
        p.hotword_weight = float(hotword_weight)
        p.alpha = float(lm.alpha) if lm is not None else 0.0
        p.beta = float(lm.beta) if lm is not None else 0.0
        p.unk_score_offset = float(lm.unk_score_offset) if lm is not None else 0.0
        p.log_base_change = LOG_BASE_CHANGE_FACTOR
        p.lm_score_boundary = int(bool(lm.score_boundary)) if lm is not None else 0
        p.first_frame = 0
        p.texts_only = 0
        p.token_frames = 0
        return p

    def _run(self, logits_list: Sequence[Any], params: B.Params, hotwords, start_states=None, hot_sets=None):
        """-> result handle. Caller must free the handle. hot_sets: per-utterance hot words (_resolve_hot)."""
        with self._call_lock:
            return self._run_locked(logits_list, params, hotwords, start_states, hot_sets)

    def _run_locked(self, logits_list: Sequence[Any], params: B.Params, hotwords, start_states=None, hot_sets=None):
        if hot_sets is None:
            self._set_hotwords(hotwords)
        batch = _Batch(logits_list, len(self._idx2vocab))
        if batch.is_device and batch.device_index is not None and batch.device_index != self._device:
            raise ValueError("the logits live on cuda:%d but this decoder was built for cuda:%d (one process per GPU: "
                             "LOCAL_RANK / CTCDEC_DEVICE pick the device)" % (batch.device_index, self._device))
        n = len(batch.ptrs)
        ptrs, frames = _c_arrays(batch)
        st_arr = None
        n_lms = len(self._members)
        if start_states is not None and n_lms > 0:
            st_arr = (B.LmState * max(n * n_lms, 1))()
            for k, s in enumerate(start_states):
                if s is None:
                    for j in range(n_lms):
                        st_arr[k * n_lms + j].length = -1
                    continue
                if n_lms > 1:  # language_model.py:488-497
                    if not isinstance(s, MultiLanguageModelState):
                        raise AssertionError(
                            f"Wrong input state type found. Expected MultiLanguageModelState, got {type(s)}")
                    if len(s.states) != n_lms:
                        raise AssertionError(
                            f"Number of states ({len(s.states)}) does not match number of language models ({n_lms}).")
                    parts = s.states
                else:
                    parts = [s]
                for j, part in enumerate(parts):
                    if not isinstance(part, KenlmState):
                        raise AssertionError(f"Wrong input state type found. Expected KenlmState, got {type(part)}")
                    st_arr[k * n_lms + j] = part.state.to_c()
        res = C.c_void_p()
        if hot_sets is not None:
            self._arm_hot_sets(hot_sets)
        self._lib.check(
            self._lib.dll.ctcdec_decode_batch(self._handle, ptrs, frames, n, batch.dtype, int(batch.is_device),
                                              C.byref(params), st_arr, C.byref(res))
        )
        ms = (C.c_double * 3)()
        self._lib.dll.ctcdec_result_timing(res, ms)
        # [frame-prune kernels, beam kernel (HIP events on the decode stream), whole native call]
        self.last_timing_ms = (float(ms[0]), float(ms[1]), float(ms[2]))
        # 1: one wavefront per utterance (beam_wave.h), 2: one workgroup per utterance (beam_core.h)
        self.last_beam_kernel = int(self._lib.dll.ctcdec_result_beam_kernel(res))
        return res

    def _unpack(self, res: C.c_void_p, with_state: bool) -> List[List[OutputBeam]]:
        pk = B.Packed()
        self._lib.check(self._lib.dll.ctcdec_result_pack(res, C.byref(pk)))
        nb, nw, nu = int(pk.n_beams), int(pk.n_words), int(pk.n_utts)
        beam_off = np.ctypeslib.as_array(pk.beam_off, shape=(nu + 1,))
        out: List[List[OutputBeam]] = []
        if nb == 0:
            return [[] for _ in range(nu)]
        has_lm = self._language_model is not None
        if not os.environ.get("CTCDEC_PY_UNPACK"):  # the same lists from one C loop (csrc/pytexts.c)
            states = None
            if with_state and has_lm:
                states = []
                for u in range(nu):
                    for k in range(int(beam_off[u]), int(beam_off[u + 1])):
                        states.append(self._beam_state(res, pk, u, k, k - int(beam_off[u])))
            frames_of = None
            if not os.environ.get("CTCDEC_EAGER_FRAMES"):  # (diagnostics / tests: plain lists of tuples built in C)
                if nw:
                    ws = np.ctypeslib.as_array(pk.word_start, shape=(nw,)).copy()
                    we = np.ctypeslib.as_array(pk.word_end, shape=(nw,)).copy()
                else:
                    ws = we = np.zeros(0, dtype=np.int32)
                frames_of = _lazy_word_frames_factory(ws, we)
            built = B.output_beams(OutputBeam, pk, states, frames_of)
            if built is not None:
                return built
        text_off = np.ctypeslib.as_array(pk.text_off, shape=(nb + 1,))
        blob = C.string_at(pk.text_blob, int(text_off[nb])) if text_off[nb] else b""
        logit = np.ctypeslib.as_array(pk.logit_score, shape=(nb,))
        lm = np.ctypeslib.as_array(pk.lm_score, shape=(nb,))
        wco = np.ctypeslib.as_array(pk.word_cnt_off, shape=(nb + 1,))
        if nw:
            wstart = np.ctypeslib.as_array(pk.word_start, shape=(nw,))
            wend = np.ctypeslib.as_array(pk.word_end, shape=(nw,))
        for u in range(nu):
            beams = []
            for k in range(int(beam_off[u]), int(beam_off[u + 1])):
                text = blob[int(text_off[k]) : int(text_off[k + 1])].decode("utf-8")
                words = text.split(" ") if text else []
                w0, w1 = int(wco[k]), int(wco[k + 1])
                frames = [(words[j], (int(wstart[w0 + j]), int(wend[w0 + j]))) for j in range(w1 - w0)]
                state = self._beam_state(res, pk, u, k, k - int(beam_off[u])) if (with_state and has_lm) else None
                beams.append(OutputBeam(text, state, frames, float(logit[k]), float(lm[k])))
            out.append(beams)
        return out

    def _beam_state(self, res, pk, u: int, k: int, j_in_utt: int) -> AbstractLMState:
        """last_lm_state of packed beam k (beam j_in_utt of utterance u)."""
        state: AbstractLMState = KenlmState(NgramState.from_c(pk.lm_state[k]))
        if len(self._members) > 1:
            parts = [state]
            for j in range(1, len(self._members)):
                cst = B.LmState()
                self._lib.check(self._lib.dll.ctcdec_result_lm_state_of(res, u, j_in_utt, j, C.byref(cst)))
                parts.append(KenlmState(NgramState.from_c(cst)))
            state = MultiLanguageModelState(parts)
        return state

    # -- public decode surface (decoder.py:730-945) ----------------------------------------------
    def decode_beams(
        self,
        logits: Any,
        beam_width: int = DEFAULT_BEAM_WIDTH,
        beam_prune_logp: float = DEFAULT_PRUNE_LOGP,
        token_min_logp: float = DEFAULT_MIN_TOKEN_LOGP,
        prune_history: bool = DEFAULT_PRUNE_BEAMS,
        hotwords: Optional[Iterable[str]] = None,
        hotword_weight: float = DEFAULT_HOTWORD_WEIGHT,
        lm_start_state: Optional[AbstractLMState] = None,
        token_frames: bool = False,
        confidence: Optional[str] = None,
    ) -> List[OutputBeam]:
        """token_frames=True: TokenOutputBeams, which also carry the frames of every token of the beam.
        confidence="mean" | "min" | "max" (implies token_frames): ConfidenceOutputBeams, which also carry the confidence of
        every token -- that fold of its label's log-probability over its frames -- and of every word."""
        self._check_logits_dimension(logits)
        fold = _confidence_fold(confidence)
        params = self._params(beam_width, beam_prune_logp, token_min_logp, prune_history, hotword_weight, 0)
        params.token_frames = fold or int(bool(token_frames))
        res = self._run([logits], params, hotwords, [lm_start_state])
        try:
            beams = self._unpack(res, True)
            return (self._with_tokens(res, beams, bool(fold)) if params.token_frames else beams)[0]
        finally:
            self._lib.dll.ctcdec_result_free(res)

    def decode(
        self,
        logits: Any,
        beam_width: int = DEFAULT_BEAM_WIDTH,
        beam_prune_logp: float = DEFAULT_PRUNE_LOGP,
        token_min_logp: float = DEFAULT_MIN_TOKEN_LOGP,
        hotwords: Optional[Iterable[str]] = None,
        hotword_weight: float = DEFAULT_HOTWORD_WEIGHT,
        lm_start_state: Optional[AbstractLMState] = None,
    ) -> str:
        self._check_logits_dimension(logits)
        # prune_history=True: only the best beam is read (decoder.py:888)
        params = self._params(beam_width, beam_prune_logp, token_min_logp, True, hotword_weight, 1)
        res = self._run([logits], params, hotwords, [lm_start_state])
        try:
            return self._unpack(res, False)[0][0].text
        finally:
            self._lib.dll.ctcdec_result_free(res)

    def decode_batch(
        self,
        pool: Any,
        logits_list: Sequence[Any],
        beam_width: int = DEFAULT_BEAM_WIDTH,
        beam_prune_logp: float = DEFAULT_PRUNE_LOGP,
        token_min_logp: float = DEFAULT_MIN_TOKEN_LOGP,
        hotwords: Optional[Iterable[str]] = None,
        hotword_weight: float = DEFAULT_HOTWORD_WEIGHT,
        token_frames: bool = False,
        confidence: Optional[str] = None,
    ) -> Any:
        """decoder.py:895-945. One device launch decodes the whole batch: a multiprocessing pool is ignored. A
        `pyctcdecode_amd.parallel.DevicePool` -- one worker process per GPU -- shards the batch over its devices.
        token_frames=True: returns (texts, TokenFrames), the frames of every token of each text as arrays.
        confidence="mean" | "min" | "max" (implies token_frames): the TokenFrames also carry ``logp``, the confidence of
        every token (ConfidenceOutputBeam.token_logp) as a float64 array."""
        fold = _confidence_fold(confidence)
        token_frames = bool(token_frames) or bool(fold)
        if getattr(logits_list, "ndim", 0) != 3:
            logits_list = list(logits_list)
        if len(logits_list) == 0:
            return ([], self._empty_token_frames(bool(fold))) if token_frames else []
        if type(pool).__name__ == "DevicePool":
            kw = dict(confidence=confidence) if fold else dict(token_frames=True) if token_frames else {}
            return pool.decode_batch(logits_list, beam_width=beam_width, beam_prune_logp=beam_prune_logp,
                                     token_min_logp=token_min_logp, hotwords=hotwords, hotword_weight=hotword_weight, **kw)
        hotwords, hotword_weight, hot_sets = self._resolve_hot(hotwords, hotword_weight, len(logits_list))
        params = self._params(beam_width, beam_prune_logp, token_min_logp, True, hotword_weight, 1)
        if token_frames:  # (the best beam's emission list comes back: one host pass gives its text and its tokens)
            params.token_frames = fold or 1
        else:
            params.texts_only = 1  # (the kernels write the texts themselves: no emission lists to copy back and replay)
        res = self._run(logits_list, params, hotwords, hot_sets=hot_sets)
        try:
            texts = self._texts(res)
            return (texts, self._token_frames(res, len(texts), bool(fold))) if token_frames else texts
        finally:
            self._lib.dll.ctcdec_result_free(res)

    def _empty_token_frames(self, with_logp: bool = False) -> TokenFrames:
        z = np.zeros(0, dtype=np.int32)
        return TokenFrames(z, z.copy(), z.copy(), np.zeros(1, dtype=np.int64), self._alphabet.labels,
                           np.zeros(0, dtype=np.float64) if with_logp else None)

    def _token_frames(self, res, n_beams: int, with_logp: bool = False) -> TokenFrames:
        """The token frames of all beams of a result (ctcdec_result_token_frames), copied into numpy arrays; with_logp: and
        their confidences (ctcdec_result_token_logp)."""
        off_p, lab_p, st_p, en_p = (C.POINTER(C.c_int64)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(),
                                    C.POINTER(C.c_int32)())
        n = C.c_int64()
        self._lib.check(self._lib.dll.ctcdec_result_token_frames(res, C.byref(off_p), C.byref(lab_p), C.byref(st_p),
                                                                 C.byref(en_p), C.byref(n)))
        nt = int(n.value)
        offsets = np.ctypeslib.as_array(off_p, shape=(n_beams + 1,)).copy()
        if nt:
            arrs = [np.ctypeslib.as_array(q, shape=(nt,)).copy() for q in (lab_p, st_p, en_p)]
        else:
            arrs = [np.zeros(0, dtype=np.int32) for _ in range(3)]
        logp = None
        if with_logp:
            logp = self._token_logp(res)
            if len(logp) != nt:
                raise B.NativeError("token confidences and token frames differ in number")
        return TokenFrames(arrs[0], arrs[1], arrs[2], offsets, self._alphabet.labels, logp)

    def _token_logp(self, res) -> np.ndarray:
        """The token confidences of all beams of a result (ctcdec_result_token_logp), copied into a float64 array."""
        lp_p, n = C.POINTER(C.c_double)(), C.c_int64()
        self._lib.check(self._lib.dll.ctcdec_result_token_logp(res, C.byref(lp_p), C.byref(n)))
        nt = int(n.value)
        return np.ctypeslib.as_array(lp_p, shape=(nt,)).copy() if nt else np.zeros(0, dtype=np.float64)

    def _with_tokens(self, res, beams: List[List[OutputBeam]], with_logp: bool = False) -> List[List[TokenOutputBeam]]:
        tf = self._token_frames(res, sum(len(bs) for bs in beams), with_logp)
        out, k = [], 0
        for bs in beams:
            row = []
            for b in bs:
                toks = tf.of(k)
                if with_logp:
                    lps = tf.logp_of(k)
                    row.append(ConfidenceOutputBeam(b.text, b.last_lm_state, b.text_frames, b.logit_score, b.lm_score, toks,
                                                    lps, _word_logps(b.text_frames, toks, lps)))
                else:
                    row.append(TokenOutputBeam(b.text, b.last_lm_state, b.text_frames, b.logit_score, b.lm_score, toks))
                k += 1
            out.append(row)
        return out

    def _texts(self, res) -> List[str]:
        """The texts of all beams of a result (utterance-major)."""
        texts = B.texts_of(self._lib, res)  # (one str per block of the library's memory, built in C)
        if texts is not None:
            return texts
        if self._texts_sep is not None:  # one split instead of one slice per utterance (0.7 -> 0.15 ms at 4096)
            blob_p, nbytes, n = C.c_void_p(), C.c_int64(), C.c_int64()
            self._lib.check(self._lib.dll.ctcdec_result_texts_joined(res, self._texts_sep, C.byref(blob_p), C.byref(nbytes),
                                                                     C.byref(n)))
            if n.value == 0:
                return []
            parts = B.split_texts(blob_p, int(nbytes.value), int(n.value), self._texts_sep)
            if len(parts) == n.value:
                return parts
        blob_p, off_p, n = C.c_void_p(), C.POINTER(C.c_int64)(), C.c_int64()
        self._lib.check(self._lib.dll.ctcdec_result_texts(res, C.byref(blob_p), C.byref(off_p), C.byref(n)))
        nb = int(n.value)
        text_off = np.ctypeslib.as_array(off_p, shape=(nb + 1,))
        blob = C.string_at(blob_p, int(text_off[nb])) if text_off[nb] else b""
        off = text_off.tolist()
        if blob.isascii():  # byte offsets == character offsets: decode once, slice the str
            text = blob.decode("ascii")
            return [text[off[k] : off[k + 1]] for k in range(nb)]
        return [blob[off[k] : off[k + 1]].decode("utf-8") for k in range(nb)]

    def decode_beams_batch(
        self,
        pool: Any,
        logits_list: Sequence[Any],
        beam_width: int = DEFAULT_BEAM_WIDTH,
        beam_prune_logp: float = DEFAULT_PRUNE_LOGP,
        token_min_logp: float = DEFAULT_MIN_TOKEN_LOGP,
        prune_history: bool = DEFAULT_PRUNE_BEAMS,
        hotwords: Optional[Iterable[str]] = None,
        hotword_weight: float = DEFAULT_HOTWORD_WEIGHT,
        token_frames: bool = False,
        confidence: Optional[str] = None,
    ) -> List[List[OutputBeam]]:
        """decoder.py:801-857. Beams carry ``last_lm_state=None`` like the reference's mp-safe beams. ``pool``: see decode_batch.
        token_frames=True: TokenOutputBeams, which also carry the frames of every token of the beam.
        confidence="mean" | "min" | "max" (implies token_frames): ConfidenceOutputBeams, see decode_beams."""
        fold = _confidence_fold(confidence)
        token_frames = bool(token_frames) or bool(fold)
        logits_list = list(logits_list)
        for logits in logits_list:
            self._check_logits_dimension(logits)
        if len(logits_list) == 0:
            return []
        if type(pool).__name__ == "DevicePool":
            kw = dict(confidence=confidence) if fold else dict(token_frames=True) if token_frames else {}
            return pool.decode_beams_batch(logits_list, beam_width=beam_width, beam_prune_logp=beam_prune_logp,
                                           token_min_logp=token_min_logp, prune_history=prune_history, hotwords=hotwords,
                                           hotword_weight=hotword_weight, **kw)
        hotwords, hotword_weight, hot_sets = self._resolve_hot(hotwords, hotword_weight, len(logits_list))
        params = self._params(beam_width, beam_prune_logp, token_min_logp, prune_history, hotword_weight, 0)
        params.token_frames = fold or int(token_frames)
        res = self._run(logits_list, params, hotwords, hot_sets=hot_sets)
        try:
            beams = self._unpack(res, False)
            return self._with_tokens(res, beams, bool(fold)) if token_frames else beams
        finally:
            self._lib.dll.ctcdec_result_free(res)

    # -- forced alignment (no reference analogue; DESIGN.md, "Forced alignment") ------------------------
    def _target_of_text(self, text: str) -> List[int]:
        """The label ids of a whitespace-normalised text under a character alphabet: its characters, the space label
        between words."""
        out = []
        for ch in " ".join(text.split()):
            idx = self._vocab2idx.get(ch)
            if idx is None or ch == "":
                raise ValueError("character %r of the text %r is not a label of the alphabet" % (ch, text))
            out.append(idx)
        return out

    def _words_of_target(self, ids: Sequence[int]):
        """-> (text, kept, words): the positions of the target that are tokens (all but the space label of a character
        alphabet) and, per word, (its string, first kept index, one past its last kept index)."""
        labels = self._labels_list
        kept, words, cur, lo = [], [], [], 0
        from .alphabet import BPE_TOKEN

        def close():
            nonlocal cur, lo
            if cur:
                words.append(("".join(cur), lo, len(kept)))
            cur, lo = [], len(kept)

        force = False
        for pos, c in enumerate(ids):
            lab = labels[c]
            if not self._is_bpe:
                if lab == " ":
                    close()
                    continue
                cur.append(lab)
            else:
                if force or lab.startswith(BPE_TOKEN):
                    close()
                force = len(lab) > 1 and lab.endswith(BPE_TOKEN)
                cur.append(lab.strip(BPE_TOKEN))
            kept.append(pos)
        close()
        return " ".join(w for w, _, _ in words), kept, words

    def _one_target_each(self, what: str, logits_list: Any, texts, tokens, max_labels: int = ALIGN_MAX_LABELS):
        """-> (logits_list, targets): the checks align_batch and posteriors_batch make of their arguments before anything is
        staged -- one target per utterance, as a text (character alphabets) or as label ids, of at most ``max_labels``."""
        if (texts is None) == (tokens is None):
            raise ValueError("%s: give exactly one of texts and tokens" % what)
        if texts is not None and self._is_bpe:
            raise ValueError("a text has many segmentations under a BPE alphabet: give the target as tokens=")
        if getattr(logits_list, "ndim", 0) != 3:
            logits_list = list(logits_list)
        n = len(logits_list)
        given = texts if texts is not None else tokens
        if isinstance(given, str) or len(given) != n:
            raise ValueError("%s: %d targets for %d utterances" % (what, 1 if isinstance(given, str) else len(given), n))
        blank, n_labels = self._vocab2idx[""], len(self._labels_list)
        targets: List[List[int]] = []
        for u, g in enumerate(given):
            if texts is not None:
                if not isinstance(g, str):
                    raise ValueError("%s: texts[%d] is not a str" % (what, u))
                ids = self._target_of_text(g)
            else:
                ids = []
                for c in g:
                    if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 0 <= int(c) < n_labels or int(c) == blank:
                        raise ValueError("%s: tokens[%d] holds %r: not a label id in [0, %d) other than the blank (%d)"
                                         % (what, u, c, n_labels, blank))
                    ids.append(int(c))
            if len(ids) > max_labels:
                raise ValueError("%s: utterance %d has %d target labels, above the limit of %d labels per utterance"
                                 % (what, u, len(ids), max_labels))
            targets.append(ids)
        return logits_list, targets

    def _stage_transcript_call(self, logits_list: Any):
        """-> (batch, frames, ptrs, c_utts): what every transcript call stages, under the call lock -- the utterances as a _Batch,
        on this decoder's device if on one, their frame counts and matrix pointers as arrays for the native call, and these
        as the call's two leading arguments (_c_utts)."""
        batch = _Batch(logits_list, len(self._labels_list))
        if batch.is_device and batch.device_index is not None and batch.device_index != self._device:
            raise ValueError("the logits live on cuda:%d but this decoder was built for cuda:%d (one process per GPU: "
                             "LOCAL_RANK / CTCDEC_DEVICE pick the device)" % (batch.device_index, self._device))
        frames, ptrs = np.ascontiguousarray(batch.frames, dtype=np.int32), np.ascontiguousarray(batch.ptrs, dtype=np.uint64)
        return batch, frames, ptrs, self._c_utts(ptrs, frames)

    @staticmethod
    def _c_utts(ptrs: np.ndarray, frames: np.ndarray):
        """-> the two leading arguments of every native transcript call: the matrix pointers and the frame counts"""
        return ptrs.ctypes.data_as(C.POINTER(C.c_void_p)), frames.ctypes.data_as(C.POINTER(C.c_int32))

    @staticmethod
    def _frames_needed(ids: Sequence[int]) -> int:
        """The fewest frames a path through the labels takes: one each, and a blank between adjacent equal ones."""
        return len(ids) + sum(1 for a, b in zip(ids, ids[1:]) if a == b)

    def _feasible(self, what: str, frames, labels: Sequence[Sequence[int]], table_bytes, budget: int, strict: bool,
                  table_name: str = "table", path_name: str = "alignment") -> List[int]:
        """-> the utterances that have a path for their labels. One whose table, of ``table_bytes(frames, labels)`` bytes, is
        above the budget of a launch is a ValueError, and so are, when ``strict``, the utterances without a path. The
        messages call the table and the path by the call's own words."""
        keep, bad = [], []
        for u, ids in enumerate(labels):
            (keep if int(frames[u]) >= self._frames_needed(ids) else bad).append(u)
            table = table_bytes(int(frames[u]), len(ids))
            if table > budget:
                raise ValueError("%s: utterance %d needs a %s of %d bytes, above the memory budget of %d bytes of one launch"
                                 % (what, u, table_name, table, budget))
        if bad and strict:
            raise ValueError("%s: no %s for utterances %s: fewer frames than target labels plus adjacent equal labels"
                             % (what, path_name, bad))
        return keep

    @staticmethod
    def _bp_table_bytes(frames: int, n_labels: int) -> int:
        """A byte of back-pointers per frame and group of four states (ctc_viterbi, ctc_viterbi_gaps)"""
        return frames * ((2 * n_labels + 1 + 3) // 4)

    @staticmethod
    def _state_table_bytes(frames: int, n_labels: int) -> int:
        """32 bytes of states per frame and group of four states (ctc_posteriors)"""
        return 32 * frames * ((2 * n_labels + 1 + 3) // 4)

    @staticmethod
    def _pack_ids(seqs: Sequence[Sequence[int]]):
        """-> (flat, off): the id lists end to end as int32 (one 0 where there is none: never read) and where each starts."""
        flat = np.fromiter(itertools.chain.from_iterable(seqs), dtype=np.int32)
        off = np.zeros(len(seqs) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(ids) for ids in seqs])
        return (flat if len(flat) else np.zeros(1, dtype=np.int32)), off

    @classmethod
    def _pack_items(cls, items: Sequence[Sequence[Sequence[int]]]):
        """-> (flat, label_off, item_off, n_items): _many_targets_each's id lists of every utterance end to end (_pack_ids),
        and where each utterance's items start among them."""
        flat_items = [ids for cur in items for ids in cur]
        flat, label_off = cls._pack_ids(flat_items)
        item_off = np.zeros(len(items) + 1, dtype=np.int64)
        item_off[1:] = np.cumsum([len(cur) for cur in items])
        return flat, label_off, item_off, len(flat_items)

    def align(self, logits: Any, text: Optional[str] = None, tokens: Optional[Sequence[int]] = None,
              confidence: Optional[str] = None) -> "AlignedText":
        """Forced alignment of one utterance: align_batch of a batch of one (a ValueError when no path exists)."""
        self._check_logits_dimension(logits)
        return self.align_batch([logits], None if text is None else [text], tokens=None if tokens is None else [tokens],
                                confidence=confidence)[0]

    def align_batch(self, logits_list: Any, texts: Optional[Sequence[str]] = None, tokens: Optional[Sequence[Sequence[int]]] = None,
                    confidence: Optional[str] = None, strict: bool = True, _bp_budget: int = 0) -> List[Optional["AlignedText"]]:
        """Where each known transcript lies in its utterance, in one native call: per utterance the best CTC path for its
        target (row_lse + ctc_viterbi, csrc/ctc_align_hip.hip), as AlignedText. ``logits_list`` is what decode_batch takes,
        and probabilities are told from logits by the same rule. ``texts`` (character alphabets): the target is the
        characters of the whitespace-normalised text; ``tokens``: label ids per utterance, the only form for BPE alphabets.
        An utterance with fewer frames than target labels plus adjacent equal labels has no path: ``strict=True`` raises a
        ValueError that lists them, ``strict=False`` returns None in their place."""
        fold = _confidence_fold(confidence)
        logits_list, targets = self._one_target_each("align", logits_list, texts, tokens)
        out, stats = self._aligned_texts("align", logits_list, targets, fold, strict, int(_bp_budget), None)
        if stats is not None:
            # [classification (frame-prune kernels), row_lse, ctc_viterbi (HIP events), whole native call]; launches made
            self.last_align_timing_ms, self.last_align_launches, _plan = stats
        return out

    def _aligned_texts(self, what: str, logits_list: Any, targets: List[List[int]], fold: int, strict: bool, bp_budget: int,
                       segment_frames: Optional[int]):
        """-> (the AlignedText of every utterance, None for one without a path; (timing ms, launches, plan) of the native call,
        None when none was made): the checked targets through ctcdec_align_batch (``segment_frames`` None) or
        ctcdec_align_long_batch, and the words formed from the result."""
        n = len(targets)
        if n == 0:
            return [], None
        budget = bp_budget or ALIGN_BP_BUDGET
        with self._call_lock:
            batch, frames, ptrs, _ = self._stage_transcript_call(logits_list)
            if segment_frames is None:
                keep = self._feasible(what, frames, targets, self._bp_table_bytes, budget, strict, "back-pointer table", "path")
            else:
                keep = self._feasible(what, frames, targets, lambda T, L: self._align_long_plan(T, L, budget, segment_frames)[2],
                                      budget, strict, "plan (segment table, checkpoints, columns)", "path")
            out: List[Optional[AlignedText]] = [None] * n
            if not keep:
                return out, None
            k_ptrs = np.ascontiguousarray(ptrs[keep])
            k_frames = np.ascontiguousarray(frames[keep])
            flat, off = self._pack_ids([targets[u] for u in keep])
            res = C.c_void_p()
            lib = self._lib
            head = (self._handle, *self._c_utts(k_ptrs, k_frames), len(keep), batch.dtype, int(batch.is_device),
                    flat.ctypes.data_as(C.POINTER(C.c_int32)), B.off_ptr(off), fold, bp_budget)
            if segment_frames is None:
                lib.check(lib.dll.ctcdec_align_batch(*head, C.byref(res)))
            else:
                lib.check(lib.dll.ctcdec_align_long_batch(*head, segment_frames, C.byref(res)))
            try:
                po, pp, ps, nu = C.POINTER(C.c_int64)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_double)(), C.c_int64()
                lib.check(lib.dll.ctcdec_alignment_paths(res, C.byref(po), C.byref(pp), C.byref(ps), C.byref(nu)))
                to, tl, ts, te, tp, nt = (C.POINTER(C.c_int64)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(),
                                          C.POINTER(C.c_int32)(), C.POINTER(C.c_double)(), C.c_int64())
                lib.check(lib.dll.ctcdec_alignment_tokens(res, C.byref(to), C.byref(tl), C.byref(ts), C.byref(te), C.byref(tp),
                                                          C.byref(nt)))
                if int(nu.value) != len(keep) or int(nt.value) != int(off[-1]):
                    raise B.NativeError("the alignment holds another number of utterances or tokens than was asked for")
                path_off = np.ctypeslib.as_array(po, shape=(len(keep) + 1,))
                total = int(path_off[-1])
                path = np.ctypeslib.as_array(pp, shape=(total,)).copy() if total else np.zeros(0, dtype=np.int32)
                score = np.ctypeslib.as_array(ps, shape=(len(keep),)).tolist()
                ntok = int(nt.value)
                start = np.ctypeslib.as_array(ts, shape=(ntok,)).tolist() if ntok else []
                end = np.ctypeslib.as_array(te, shape=(ntok,)).tolist() if ntok else []
                logp = np.ctypeslib.as_array(tp, shape=(ntok,)).tolist() if ntok and fold else []
                ms, launches = (C.c_double * 4)(), C.c_int32()
                lib.dll.ctcdec_alignment_timing(res, ms, C.byref(launches))
                sf, ns, npl = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.c_int64()
                lib.check(lib.dll.ctcdec_alignment_plan(res, C.byref(sf), C.byref(ns), C.byref(npl)))
                plan = [(int(sf[j]), int(ns[j])) for j in range(int(npl.value))]
                stats = (tuple(float(v) for v in ms), int(launches.value), plan)
                path_off = path_off.tolist()
            finally:
                lib.dll.ctcdec_alignment_free(res)
            labels = self._labels_list
            for j, u in enumerate(keep):
                ids, o = targets[u], int(off[j])
                text, kept, words = self._words_of_target(ids)
                tok = [(labels[ids[k]], (start[o + k], end[o + k])) for k in kept]
                wf = [(w, (tok[lo][1][0], tok[hi - 1][1][1])) for w, lo, hi in words]
                tlp = wlp = None
                if fold:
                    tlp = [logp[o + k] for k in kept]
                    wlp = [min(tlp[lo:hi]) for _w, lo, hi in words]
                out[u] = AlignedText(text, path[path_off[j]:path_off[j + 1]].copy(), float(score[j]), tok, wf, tlp, wlp)
            return out, stats

    # -- forced alignment of long transcripts (no reference analogue; DESIGN.md, "Forced alignment of long transcripts") ------
    @staticmethod
    def _align_long_plan(frames: int, n_labels: int, budget: int, segment_frames: int) -> Tuple[int, int, int]:
        """-> (K, n, bytes): how ctcdec_align_long_batch cuts an utterance (long_plan, csrc/api_transcript.cpp, the same rule):
        segments of K frames, n = ceil((frames - 1) / K) of them, and the bytes of one segment's back-pointers, a checkpoint
        per segment when there is more than one, and the two score columns."""
        nch = (2 * n_labels + 1 + 3) // 4

        def of(K):
            n = (frames - 2) // K + 1 if frames > 1 else 0
            return K, n, K * nch + (32 * nch * n if n > 1 else 0) + 64 * nch

        if frames <= 0:
            return 0, 0, 0
        if segment_frames > 0:
            return of(min(segment_frames, frames))
        whole = of(frames)
        if whole[2] <= budget:
            return whole
        K = math.isqrt(32 * frames)
        return of(min(K if K * K == 32 * frames else K + 1, frames))

    def align_long(self, logits: Any, text: Optional[str] = None, tokens: Optional[Sequence[int]] = None,
                   confidence: Optional[str] = None) -> "AlignedText":
        """Forced alignment of one long utterance: align_long_batch of a batch of one (a ValueError when no path exists)."""
        if isinstance(logits, (_ResidentBeams, _DeviceStreams)):
            raise NotImplementedError("align_long reads an utterance's matrix; the frames a stream has consumed are not kept")
        self._check_logits_dimension(logits)
        return self.align_long_batch([logits], None if text is None else [text], tokens=None if tokens is None else [tokens],
                                     confidence=confidence)[0]

    def align_long_batch(self, logits_list: Any, texts: Optional[Sequence[str]] = None,
                         tokens: Optional[Sequence[Sequence[int]]] = None, confidence: Optional[str] = None, strict: bool = True,
                         _bp_budget: int = 0, _segment_frames: int = 0) -> List[Optional["AlignedText"]]:
        """align_batch for a lecture against its script: up to 1048575 target labels per utterance instead of 2047, and no
        back-pointer table of all frames (row_lse + ctc_viterbi_long, csrc/ctc_align_hip.hip). Arguments, targets, the
        probabilities-or-logits rule and ``strict`` are align_batch's, and for every input align_batch accepts the result is
        align_batch's, bit for bit. An utterance whose whole table fits the memory budget of a launch takes one pass; a longer
        one is cut into segments of about sqrt(32 T) frames and takes two: one that keeps the score column every segment
        starts from, one that fills and traces back one segment's table at a time, last segment first. The score columns
        live in device memory, so align_batch stays the faster call for targets it accepts. ``last_align_long_plan`` holds
        (segment_frames, n_segments) of every utterance aligned."""
        if isinstance(logits_list, (_ResidentBeams, _DeviceStreams)) or (
                isinstance(logits_list, (list, tuple)) and any(isinstance(x, (_ResidentBeams, _DeviceStreams)) for x in logits_list)):
            raise NotImplementedError("align_long_batch reads utterances' matrices; the frames a stream has consumed are not kept")
        fold = _confidence_fold(confidence)
        if isinstance(_segment_frames, bool) or not isinstance(_segment_frames, (int, np.integer)) or not 0 <= int(_segment_frames) < 2 ** 31:
            raise ValueError("align_long: _segment_frames must be an int >= 0 (0: the library plans), not %r" % (_segment_frames,))
        logits_list, targets = self._one_target_each("align_long", logits_list, texts, tokens, ALIGN_LONG_MAX_LABELS)
        out, stats = self._aligned_texts("align_long", logits_list, targets, fold, strict, int(_bp_budget), int(_segment_frames))
        if stats is not None:
            self.last_align_long_timing_ms, self.last_align_long_launches, self.last_align_long_plan = stats
        return out

    # -- alignment with gaps (no reference analogue; DESIGN.md, "Alignment with gaps") --------------------
    def _gapped_targets(self, what: str, logits_list: Any, texts, tokens, gap: str):
        """-> (logits_list, items): the checks align_gaps_batch makes of its arguments before anything is staged -- one
        target per utterance, as a text (character alphabets) or as label ids, -1 standing for a gap; adjacent gaps merged."""
        if not isinstance(gap, str) or gap == "" or gap.split() != [gap]:
            raise ValueError("%s: the gap marker %r must be a non-empty string without whitespace" % (what, gap))
        if gap in self._vocab2idx:
            raise ValueError("%s: the gap marker %r is a label of the alphabet: choose another with gap=" % (what, gap))
        if (texts is None) == (tokens is None):
            raise ValueError("%s: give exactly one of texts and tokens" % what)
        if texts is not None and self._is_bpe:
            raise ValueError("a text has many segmentations under a BPE alphabet: give the target as tokens=")
        if getattr(logits_list, "ndim", 0) != 3:
            logits_list = list(logits_list)
        n = len(logits_list)
        given = texts if texts is not None else tokens
        if isinstance(given, str) or len(given) != n:
            raise ValueError("%s: %d targets for %d utterances" % (what, 1 if isinstance(given, str) else len(given), n))
        blank, n_labels, space = self._vocab2idx[""], len(self._labels_list), self._vocab2idx.get(" ")
        targets: List[List[int]] = []
        for u, g in enumerate(given):
            ids: List[int] = []
            if texts is not None:
                if not isinstance(g, str):
                    raise ValueError("%s: texts[%d] is not a str" % (what, u))
                for word in g.split():
                    if word == gap:
                        if not ids or ids[-1] != -1:  # (repeated markers are one gap)
                            ids.append(-1)
                        continue
                    if ids and ids[-1] != -1:  # (the space label between two words; a gap absorbs the ones next to it)
                        if space is None:
                            raise ValueError("character ' ' of the text %r is not a label of the alphabet" % g)
                        ids.append(space)
                    ids.extend(self._target_of_text(word))
            else:
                for c in g:
                    if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not -1 <= int(c) < n_labels or int(c) == blank:
                        raise ValueError("%s: tokens[%d] holds %r: not a label id in [0, %d) other than the blank (%d), nor -1 for "
                                         "a gap" % (what, u, c, n_labels, blank))
                    if int(c) == -1 and ids and ids[-1] == -1:
                        continue
                    ids.append(int(c))
            n_lab = sum(1 for c in ids if c != -1)
            if n_lab == 0:
                raise ValueError("%s: the target of utterance %d has no label: a gap alone aligns to everything" % (what, u))
            if n_lab > ALIGN_MAX_LABELS:
                raise ValueError("%s: utterance %d has %d target labels, above the limit of %d labels per utterance"
                                 % (what, u, n_lab, ALIGN_MAX_LABELS))
            targets.append(ids)
        return logits_list, targets

    def align_gaps(self, logits: Any, text: Optional[str] = None, tokens: Optional[Sequence[int]] = None, gap: str = "*",
                   confidence: Optional[str] = None) -> "GappedAlignment":
        """Alignment of one utterance to a transcript with gaps: align_gaps_batch of a batch of one."""
        self._check_logits_dimension(logits)
        return self.align_gaps_batch([logits], None if text is None else [text], tokens=None if tokens is None else [tokens],
                                     gap=gap, confidence=confidence)[0]

    def align_gaps_batch(self, logits_list: Any, texts: Optional[Sequence[str]] = None,
                         tokens: Optional[Sequence[Sequence[int]]] = None, gap: str = "*", confidence: Optional[str] = None,
                         strict: bool = True, _bp_budget: int = 0) -> List[Optional["GappedAlignment"]]:
        """align_batch for transcripts that do not cover all of the audio, in one native call (row_lse_max +
        ctc_viterbi_gaps, csrc/ctc_align_hip.hip), as GappedAlignment. In ``texts`` (character alphabets) a
        whitespace-delimited word equal to ``gap`` is a gap: ``"* bugs * bunny"`` is something untranscribed, "bugs",
        something untranscribed, "bunny" and then the end of the audio. The space labels that would stand next to a gap are
        dropped -- the gap absorbs them --, and repeated markers are one gap. In ``tokens`` -1 is a gap. A gap takes, frame
        by frame, the best log-probability any label or the blank has, so it costs what the best unconstrained path would
        pay for its frames; it may be empty wherever a blank may be skipped. A target without gaps gives align_batch's
        result. ``strict`` and the feasibility bound (frames >= labels plus adjacent equal labels) are align_batch's."""
        fold = _confidence_fold(confidence)
        logits_list, targets = self._gapped_targets("align_gaps", logits_list, texts, tokens, gap)
        n = len(targets)
        if n == 0:
            return []
        with self._call_lock:
            batch, frames, ptrs, _ = self._stage_transcript_call(logits_list)
            labels_only = [[c for c in items if c != -1] for items in targets]
            keep = self._feasible("align_gaps", frames, labels_only, self._bp_table_bytes, int(_bp_budget) or ALIGN_BP_BUDGET, strict,
                                  "back-pointer table", "path")
            out: List[Optional[GappedAlignment]] = [None] * n
            if not keep:
                return out
            k_ptrs = np.ascontiguousarray(ptrs[keep])
            k_frames = np.ascontiguousarray(frames[keep])
            flat, off = self._pack_ids([targets[u] for u in keep])
            res = C.c_void_p()
            lib = self._lib
            lib.check(lib.dll.ctcdec_align_gaps_batch(
                self._handle, *self._c_utts(k_ptrs, k_frames),
                len(keep), batch.dtype, int(batch.is_device), flat.ctypes.data_as(C.POINTER(C.c_int32)), B.off_ptr(off), fold,
                int(_bp_budget), C.byref(res)))
            try:
                po, pp, ps, nu = C.POINTER(C.c_int64)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_double)(), C.c_int64()
                lib.check(lib.dll.ctcdec_alignment_paths(res, C.byref(po), C.byref(pp), C.byref(ps), C.byref(nu)))
                to, tl, ts, te, tp, nt = (C.POINTER(C.c_int64)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(),
                                          C.POINTER(C.c_int32)(), C.POINTER(C.c_double)(), C.c_int64())
                lib.check(lib.dll.ctcdec_alignment_tokens(res, C.byref(to), C.byref(tl), C.byref(ts), C.byref(te), C.byref(tp),
                                                          C.byref(nt)))
                go, gs, ge, gl, ng = (C.POINTER(C.c_int64)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(),
                                      C.POINTER(C.c_double)(), C.c_int64())
                lib.check(lib.dll.ctcdec_alignment_gaps(res, C.byref(go), C.byref(gs), C.byref(ge), C.byref(gl), C.byref(ng)))
                n_lab = sum(1 for u in keep for c in targets[u] if c != -1)
                n_gap = int(off[-1]) - n_lab
                if int(nu.value) != len(keep) or int(nt.value) != n_lab or int(ng.value) != n_gap:
                    raise B.NativeError("the alignment holds another number of utterances, tokens or gaps than was asked for")
                path_off = np.ctypeslib.as_array(po, shape=(len(keep) + 1,)).tolist()
                total = int(path_off[-1])
                path = np.ctypeslib.as_array(pp, shape=(total,)).copy()
                score = np.ctypeslib.as_array(ps, shape=(len(keep),)).tolist()
                tok_off = np.ctypeslib.as_array(to, shape=(len(keep) + 1,)).tolist()
                start = np.ctypeslib.as_array(ts, shape=(n_lab,)).tolist()
                end = np.ctypeslib.as_array(te, shape=(n_lab,)).tolist()
                logp = np.ctypeslib.as_array(tp, shape=(n_lab,)).tolist() if fold else []
                gap_off = np.ctypeslib.as_array(go, shape=(len(keep) + 1,)).tolist()
                g_start = np.ctypeslib.as_array(gs, shape=(n_gap,)).tolist() if n_gap else []
                g_end = np.ctypeslib.as_array(ge, shape=(n_gap,)).tolist() if n_gap else []
                g_logp = np.ctypeslib.as_array(gl, shape=(n_gap,)).tolist() if n_gap else []
                ms, launches = (C.c_double * 4)(), C.c_int32()
                lib.dll.ctcdec_alignment_timing(res, ms, C.byref(launches))
                # [classification (frame-prune kernels), row_lse_max, ctc_viterbi_gaps (HIP events), whole native call]
                self.last_align_gaps_timing_ms = tuple(float(v) for v in ms)
                self.last_align_gaps_launches = int(launches.value)
            finally:
                lib.dll.ctcdec_alignment_free(res)
            labels = self._labels_list
            for j, u in enumerate(keep):
                items, o = targets[u], tok_off[j]
                # the runs of labels between the gaps: each has its own words (a gap ends a word)
                parts, tok, wf, tlp, wlp, run = [], [], [], [], [], []
                for c in items + [-1]:
                    if c != -1:
                        run.append(c)
                        continue
                    if run:
                        text, kept, words = self._words_of_target(run)
                        base = len(tok)
                        tok.extend((labels[run[k]], (start[o + k], end[o + k])) for k in kept)
                        wf.extend((w, (tok[base + lo][1][0], tok[base + hi - 1][1][1])) for w, lo, hi in words)
                        if fold:
                            tlp.extend(logp[o + k] for k in kept)
                            wlp.extend(min(tlp[base + lo:base + hi]) for _w, lo, hi in words)
                        if text:
                            parts.append(text)
                        o += len(run)
                        run = []
                    parts.append(gap)
                parts.pop()  # (the sentinel's)
                g0, g1 = gap_off[j], gap_off[j + 1]
                out[u] = GappedAlignment(" ".join(parts), list(items), path[path_off[j]:path_off[j + 1]].copy(), float(score[j]), tok,
                                         wf, list(zip(g_start[g0:g1], g_end[g0:g1])), g_logp[g0:g1], tlp if fold else None,
                                         wlp if fold else None)
            return out

    # -- greedy decode (no reference analogue; DESIGN.md, "Greedy decode") ---------------------------------
    def _greedy_call(self, logits_list: Any, fold: int):
        """-> (texts, offsets, label, start, end, logp, score): one ctcdec_greedy_batch call's results copied out -- every
        token of every utterance (the space label of a character alphabet included) as arrays, utterance u's at
        ``[offsets[u], offsets[u + 1])``; ``logp`` and ``score`` are None without a fold."""
        with self._call_lock:
            batch, frames, ptrs, c_utts = self._stage_transcript_call(logits_list)
            n = len(frames)
            res = C.c_void_p()
            lib = self._lib
            lib.check(lib.dll.ctcdec_greedy_batch(
                self._handle, *c_utts, n,
                batch.dtype, int(batch.is_device), fold, C.byref(res)))
            try:
                blob_p, off_p, nu = C.c_void_p(), C.POINTER(C.c_int64)(), C.c_int64()
                lib.check(lib.dll.ctcdec_greedy_texts(res, C.byref(blob_p), C.byref(off_p), C.byref(nu)))
                to, tl, ts, te, tp, nt = (C.POINTER(C.c_int64)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(),
                                          C.POINTER(C.c_int32)(), C.POINTER(C.c_double)(), C.c_int64())
                lib.check(lib.dll.ctcdec_greedy_tokens(res, C.byref(to), C.byref(tl), C.byref(ts), C.byref(te), C.byref(tp),
                                                       C.byref(nt)))
                sp, ns = C.POINTER(C.c_double)(), C.c_int64()
                lib.check(lib.dll.ctcdec_greedy_scores(res, C.byref(sp), C.byref(ns)))
                if int(nu.value) != n or int(ns.value) != n:
                    raise B.NativeError("the greedy result holds another number of utterances than was asked for")
                text_off = np.ctypeslib.as_array(off_p, shape=(n + 1,)).tolist()
                blob = C.string_at(blob_p, text_off[n]) if text_off[n] else b""
                if blob.isascii():  # byte offsets == character offsets: decode once, slice the str
                    whole = blob.decode("ascii")
                    texts = [whole[text_off[k]:text_off[k + 1]] for k in range(n)]
                else:
                    texts = [blob[text_off[k]:text_off[k + 1]].decode("utf-8") for k in range(n)]
                offsets = np.ctypeslib.as_array(to, shape=(n + 1,)).copy()
                ntok = int(nt.value)
                if ntok != int(offsets[-1]):
                    raise B.NativeError("the greedy result holds another number of tokens than its offsets say")
                label, start, end = (np.ctypeslib.as_array(q, shape=(ntok,)).copy() if ntok else np.zeros(0, dtype=np.int32)
                                     for q in (tl, ts, te))
                logp = score = None
                if fold:
                    logp = np.ctypeslib.as_array(tp, shape=(ntok,)).copy() if ntok else np.zeros(0, dtype=np.float64)
                    score = np.ctypeslib.as_array(sp, shape=(n,)).copy()
                ms, launches, lse_ms = (C.c_double * 4)(), C.c_int32(), C.c_double()
                lib.dll.ctcdec_greedy_timing(res, ms, C.byref(launches), C.byref(lse_ms))
                # [classification (frame-prune kernels), row_argmax / row_lse_argmax, greedy_collapse (HIP events), native call]
                self.last_greedy_timing_ms = tuple(float(v) for v in ms)
                self.last_greedy_launches = int(launches.value)
                self.last_greedy_lse_ms = float(lse_ms.value)
            finally:
                lib.dll.ctcdec_greedy_free(res)
            return texts, offsets, label, start, end, logp, score

    def decode_greedy_batch(self, logits_list: Any, token_frames: bool = False, confidence: Optional[str] = None) -> Any:
        """Greedy best-path decoding of a batch in one native call, without the language model and without a search: every
        frame takes its most probable label -- the smallest index of the row's largest entry that is not a NaN; the blank
        for a row of NaN and -inf alone --, runs of a label are one token, blanks separate tokens and are dropped
        (row_argmax + greedy_collapse, csrc/ctc_align_hip.hip: one read of the logits, compares only). ``logits_list`` is
        what decode_batch takes. Returns the texts, formed as align_batch forms an AlignedText's; with ``token_frames=True``
        ``(texts, GreedyFrames)``. ``confidence="mean" | "min" | "max"`` (implies token_frames) classifies the utterances as
        align_batch does and adds the tokens' confidences and each utterance's ``score`` (row_lse_argmax instead of
        row_argmax). There is no pool, sharded or streaming form: a DevicePool raises NotImplementedError."""
        fold = _confidence_fold(confidence)
        token_frames = bool(token_frames) or bool(fold)
        if type(logits_list).__name__ == "DevicePool":
            raise NotImplementedError("DevicePool does not shard decode_greedy_batch: call it on the process's own device")
        if getattr(logits_list, "ndim", 0) != 3:
            logits_list = list(logits_list)
        if len(logits_list) == 0:
            z = np.zeros(0, dtype=np.int32)
            empty = GreedyFrames(z, z.copy(), z.copy(), np.zeros(1, dtype=np.int64), self._alphabet.labels,
                                 np.zeros(0, dtype=np.float64) if fold else None, np.zeros(0, dtype=np.float64) if fold else None)
            return ([], empty) if token_frames else []
        texts, offsets, label, start, end, logp, score = self._greedy_call(logits_list, fold)
        if not token_frames:
            return texts
        space = None if self._is_bpe else self._vocab2idx.get(" ")
        if space is not None and len(label):  # (the space label ends a word: no token)
            keep = label != space
            offsets = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(keep, dtype=np.int64)])[offsets]
            label, start, end = label[keep], start[keep], end[keep]
            logp = logp[keep] if logp is not None else None
        return texts, GreedyFrames(label, start, end, offsets, self._alphabet.labels, logp, score)

    def decode_greedy(self, logits: Any, token_frames: bool = False, confidence: Optional[str] = None) -> Any:
        """Greedy best-path decoding of one utterance: its text, or with ``token_frames=True`` or ``confidence=...`` a
        GreedyText (decode_greedy_batch of a batch of one; word frames and confidences built as align builds them)."""
        self._check_logits_dimension(logits)
        fold = _confidence_fold(confidence)
        texts, offsets, label, start, end, logp, score = self._greedy_call([logits], fold)
        if not (token_frames or fold):
            return texts[0]
        ids, start, end = label.tolist(), start.tolist(), end.tolist()
        labels = self._labels_list
        text, kept, words = self._words_of_target(ids)
        if text != texts[0]:
            raise B.NativeError("the native text %r differs from the text of the greedy labels %r" % (texts[0], text))
        tok = [(labels[ids[k]], (start[k], end[k])) for k in kept]
        wf = [(w, (tok[lo][1][0], tok[hi - 1][1][1])) for w, lo, hi in words]
        tlp = wlp = None
        if fold:
            lp = logp.tolist()
            tlp = [lp[k] for k in kept]
            wlp = [min(tlp[lo:hi]) for _w, lo, hi in words]
        return GreedyText(text, ids, tok, wf, tlp, wlp, float(score[0]) if fold else None)

    def _many_targets_each(self, what: str, item: str, items: str, logits_list: Any, texts, tokens, ids_of_text=None):
        """The label ids of any number of given texts or token lists per utterance, checked: (logits_list, ids[u][j]).
        ``ids_of_text``: how a text becomes label ids (_target_of_text unless given)."""
        ids_of_text = ids_of_text or self._target_of_text
        if (texts is None) == (tokens is None):
            raise ValueError("%s: give exactly one of texts and tokens" % what)
        if texts is not None and self._is_bpe:
            raise ValueError("a text has many segmentations under a BPE alphabet: give the %s as tokens=" % items)
        if getattr(logits_list, "ndim", 0) != 3:
            logits_list = list(logits_list)
        n = len(logits_list)
        given = texts if texts is not None else tokens
        if not isinstance(given, str):
            given = list(given)  # (a generator has no len())
        if isinstance(given, str) or len(given) != n:
            raise ValueError("%s: %s for %d utterances, but %d utterances" % (what, items, 1 if isinstance(given, str) else len(given), n))
        blank, n_labels = self._vocab2idx[""], len(self._labels_list)
        out: List[List[List[int]]] = []
        for u, per_utt in enumerate(given):
            if isinstance(per_utt, str):
                raise ValueError("%s: utterance %d got a bare str where a sequence of %s is expected (wrap it in a "
                                 "list: a str would be read character by character)" % (what, u, items))
            cur = []
            for j, g in enumerate(per_utt):
                who = "utterance %d, %s %d" % (u, item, j)
                if texts is not None:
                    if not isinstance(g, str):
                        raise ValueError("%s: %s is not a str" % (what, who))
                    ids = ids_of_text(g)
                else:
                    if isinstance(g, str):
                        raise ValueError("%s: %s is a str, not a sequence of label ids" % (what, who))
                    ids = list(g)
                    if set(map(type, ids)) <= {int} and (not ids or (0 <= min(ids) and max(ids) < n_labels and blank not in ids)):
                        pass  # (plain ints, all in range: the check below, without a Python-level loop)
                    else:
                        for k, c in enumerate(ids):
                            if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 0 <= int(c) < n_labels or int(c) == blank:
                                raise ValueError("%s: %s holds %r: not a label id in [0, %d) other than the blank (%d)"
                                                 % (what, who, c, n_labels, blank))
                            ids[k] = int(c)
                if len(ids) > ALIGN_MAX_LABELS:
                    raise ValueError("%s: %s has %d labels, above the limit of %d labels per %s"
                                     % (what, who, len(ids), ALIGN_MAX_LABELS, item))
                cur.append(ids)
            out.append(cur)
        return logits_list, out

    # -- transcript likelihood (no reference analogue; DESIGN.md, "Transcript likelihood") ----------------
    def score(self, logits: Any, texts: Optional[Sequence[str]] = None, tokens: Optional[Sequence[Sequence[int]]] = None,
              with_lm: bool = False) -> List["ScoredText"]:
        """The likelihood of each hypothesis for one utterance: score_batch of a batch of one."""
        self._check_logits_dimension(logits)
        return self.score_batch([logits], None if texts is None else [texts], tokens=None if tokens is None else [tokens],
                                with_lm=with_lm)[0]

    def score_batch(self, logits_list: Any, texts: Optional[Sequence[Sequence[str]]] = None,
                    tokens: Optional[Sequence[Sequence[Sequence[int]]]] = None, with_lm: bool = False) -> List[List["ScoredText"]]:
        """How probable each given transcript is, in one native call: per utterance a sequence of hypotheses, per hypothesis
        the CTC forward score (row_lse once per utterance + ctc_forward / ctc_forward_wave, csrc/ctc_align_hip.hip) as
        ScoredText. ``logits_list`` is what align_batch takes; ``texts[u]`` (character alphabets) is a list of str,
        ``tokens[u]`` a list of lists of label ids, the only form for BPE alphabets. A hypothesis without an alignment --
        fewer frames than labels plus adjacent equal labels -- has ``logp == -inf``; the empty hypothesis scores the all-blank
        path. ``with_lm=True`` adds the language model's score of the text as a finished beam's (no hot words)."""
        lm = self._language_model
        if with_lm and lm is None:
            raise ValueError("score: with_lm=True needs a decoder with a language model")
        logits_list, hyps = self._many_targets_each("score", "hypothesis", "hypotheses", logits_list, texts, tokens)
        n = len(hyps)
        if n == 0:
            self.last_score_timing_ms, self.last_score_launched = (0.0, 0.0, 0.0, 0.0), (0, 0)
            return []
        kernel = _forced_kernel("CTCDEC_FORWARD_KERNEL", FORWARD_KERNELS)
        with self._call_lock:
            batch, frames, ptrs, c_utts = self._stage_transcript_call(logits_list)
            flat, target_off, hyp_off, nh = self._pack_items(hyps)
            logp = np.zeros(max(nh, 1), dtype=np.float64)
            ms, launched = (C.c_double * 4)(), (C.c_int64 * 2)()
            lib = self._lib
            lib.check(lib.dll.ctcdec_score_batch(
                self._handle, *c_utts, n,
                batch.dtype, int(batch.is_device), flat.ctypes.data_as(C.POINTER(C.c_int32)), B.off_ptr(target_off),
                B.off_ptr(hyp_off), kernel, logp.ctypes.data_as(C.POINTER(C.c_double)), ms, launched))
            # [classification (frame-prune kernels), row_lse, forward kernels (HIP events), whole native call]; hypotheses that
            # went to (ctc_forward_wave, ctc_forward)
            self.last_score_timing_ms = tuple(float(v) for v in ms)
            self.last_score_launched = (int(launched[0]), int(launched[1]))
        out: List[List[ScoredText]] = []
        h = 0
        for cur in hyps:
            res = []
            for ids in cur:
                text = self._words_of_target(ids)[0]
                lm_logp = None
                if with_lm:
                    # what the beam search adds for a finished beam (decoder.py:446-497 of the reference, without hot words)
                    state, lm_logp, words = lm.get_start_state(), 0.0, text.split()
                    for k, word in enumerate(words):
                        word_score, state = lm.score(state, word, is_last_word=k == len(words) - 1)
                        lm_logp += word_score
                lp = float(logp[h])
                res.append(ScoredText(text, list(ids), lp, lm_logp, lp + (lm_logp or 0.0)))
                h += 1
            out.append(res)
        return out

    # -- prefix scores (no reference analogue; DESIGN.md, "Prefix scores") -----------------------------------
    def _prefix_of_text(self, text: str) -> List[int]:
        """The label ids of a prefix given as text (character alphabets): _target_of_text's, and one space label more when
        the text ends in whitespace after a character -- "bugs " ends on a word boundary, "bugs" does not."""
        ids = self._target_of_text(text)
        if ids and text[-1:].isspace():
            space = self._vocab2idx.get(" ")
            if space is None:
                raise ValueError("the prefix %r ends on a word boundary, but the alphabet has no space label" % text)
            ids.append(space)
        return ids

    def prefix_scores(self, logits: Any, texts: Optional[Sequence[str]] = None,
                      tokens: Optional[Sequence[Sequence[int]]] = None) -> List["PrefixScores"]:
        """The prefix scores of each prefix for one utterance: prefix_scores_batch of a batch of one."""
        self._check_logits_dimension(logits)
        return self.prefix_scores_batch([logits], None if texts is None else [texts], tokens=None if tokens is None else [tokens])[0]

    def prefix_scores_batch(self, logits_list: Any, texts: Optional[Sequence[Sequence[str]]] = None,
                            tokens: Optional[Sequence[Sequence[Sequence[int]]]] = None) -> List[List["PrefixScores"]]:
        """What an external decoder asks at every step, in one native call: per utterance any number of prefixes, per prefix
        the CTC prefix score of every label at once as PrefixScores (row_lse once per utterance, ctc_forward_ends /
        ctc_forward_wave_ends per prefix, ctc_prefix_extend over the rows for eight prefixes of an utterance at a time;
        csrc/ctc_align_hip.hip). ``logits_list`` is what align_batch takes; ``texts[u]`` (character alphabets) is a list of
        str -- whitespace runs collapse and leading whitespace is dropped as everywhere, but trailing whitespace is kept as
        one space label --, ``tokens[u]`` a list of lists of label ids, the only form for BPE alphabets; ``[]`` or ``""`` is
        the empty prefix. The call is stateless: nothing is carried from one step's prefixes to the next's (a decoding loop,
        whose prefixes are each a parent plus one label, wants prefix_session: the same bits, O(T) per child). Host arrays give
        numpy arrays; device tensors give torch tensors on the same device, views of ``last_prefix_next``, which the
        kernels write in place."""
        logits_list, prefixes = self._many_targets_each("prefix_scores", "prefix", "prefixes", logits_list, texts, tokens,
                                                        ids_of_text=self._prefix_of_text)
        n, n_labels = len(prefixes), len(self._labels_list)
        self.last_prefix_timing_ms, self.last_prefix_launched, self.last_prefix_launches = (0.0,) * 5, (0, 0), (0, 0, 0)
        self.last_prefix_next = None
        if n == 0:
            return []
        kernel = _forced_kernel("CTCDEC_FORWARD_KERNEL", FORWARD_KERNELS)
        with self._call_lock:
            batch, frames, ptrs, c_utts = self._stage_transcript_call(logits_list)
            flat, label_off, prefix_off, nh = self._pack_items(prefixes)
            # one [prefixes, V] block of float64: for device tensors the shell makes it and the kernels fill it in place
            buf, next_ptr = None, None
            if batch.is_device and nh:
                import torch

                buf = torch.empty((nh, n_labels), dtype=torch.float64, device=batch.keep[0].device)
                next_ptr = C.c_void_p(buf.data_ptr())
            res = C.c_void_p()
            lib = self._lib
            lib.check(lib.dll.ctcdec_prefix_batch(
                self._handle, *c_utts, n,
                batch.dtype, int(batch.is_device), flat.ctypes.data_as(C.POINTER(C.c_int32)), B.off_ptr(label_off),
                B.off_ptr(prefix_off), kernel, next_ptr, C.byref(res)))
            try:
                end_p, next_p, np_, nv = C.POINTER(C.c_double)(), C.POINTER(C.c_double)(), C.c_int64(), C.c_int32()
                lib.check(lib.dll.ctcdec_prefix_scores(res, C.byref(end_p), C.byref(next_p), C.byref(np_), C.byref(nv)))
                if int(np_.value) != nh or int(nv.value) != n_labels:
                    raise B.NativeError("the prefix result holds another number of scores than was asked for")
                end = np.ctypeslib.as_array(end_p, shape=(nh,)).copy() if nh else np.zeros(0, dtype=np.float64)
                if buf is None:
                    buf = (np.ctypeslib.as_array(next_p, shape=(nh, n_labels)).copy() if nh
                           else np.zeros((0, n_labels), dtype=np.float64))
                ms, launches, launched = (C.c_double * 5)(), (C.c_int32 * 3)(), (C.c_int64 * 2)()
                lib.dll.ctcdec_prefix_timing(res, ms, launches, launched)
                # [classification (frame-prune kernels), row_lse, forward kernels with end states, ctc_prefix_extend (HIP
                # events), whole native call]; prefixes that went to (ctc_forward_wave_ends, ctc_forward_ends)
                self.last_prefix_timing_ms = tuple(float(v) for v in ms)
                self.last_prefix_launches = tuple(int(v) for v in launches)
                self.last_prefix_launched = (int(launched[0]), int(launched[1]))
            finally:
                lib.dll.ctcdec_prefix_free(res)
            if batch.is_device:
                self.last_prefix_next = buf
        space = None if self._is_bpe else self._vocab2idx.get(" ")
        rows = buf.unbind(0) if batch.is_device else list(buf)  # (every row's view in one call)
        ends = end.tolist()
        out: List[List[PrefixScores]] = []
        h = 0
        for cur in prefixes:
            got = []
            for ids in cur:
                text = self._words_of_target(ids)[0] + (" " if ids and ids[-1] == space else "")
                got.append(PrefixScores(text, list(ids), ends[h], rows[h]))
                h += 1
            out.append(got)
        return out

    def prefix_session(self, logits_list: Any, capacity: Optional[int] = None) -> "PrefixSession":
        """prefix_scores_batch for a decoding loop: a PrefixSession over the batch, in which a live prefix is extended by one
        label in O(T) and row_lse runs once. ``logits_list`` is what prefix_scores_batch takes; ``capacity`` is the number
        of prefixes that can be live at once, the utterances' empty prefixes among them (default: 64 per utterance). Every
        prefix of the session has the bits prefix_scores_batch gives for its labels ("Prefix sessions")."""
        return PrefixSession(self, logits_list, capacity)

    # -- phrase search (no reference analogue; DESIGN.md, "Phrase search") ----------------------------------
    def find(self, logits: Any, texts: Optional[Sequence[str]] = None, tokens: Optional[Sequence[Sequence[int]]] = None,
             max_hits: int = 1, min_logp: Optional[float] = None, trace: bool = False) -> List["PhraseSearch"]:
        """Where each phrase occurs in one utterance: find_batch of a batch of one."""
        if isinstance(logits, (_ResidentBeams, _DeviceStreams)):
            raise NotImplementedError("find searches an utterance's matrix; the frames a stream has consumed are not kept")
        self._check_logits_dimension(logits)
        return self.find_batch([logits], None if texts is None else [texts], tokens=None if tokens is None else [tokens],
                               max_hits=max_hits, min_logp=min_logp, trace=trace)[0]

    def find_batch(self, logits_list: Any, texts: Optional[Sequence[Sequence[str]]] = None,
                   tokens: Optional[Sequence[Sequence[Sequence[int]]]] = None, max_hits: int = 1,
                   min_logp: Optional[float] = None, trace: bool = False, _trace_budget: int = 0) -> List[List["PhraseSearch"]]:
        """Does each phrase occur somewhere in its utterance, where, and how well, in one native call: per utterance a
        sequence of phrases, per phrase a PhraseSearch (row_lse once per utterance + ctc_find / ctc_find_wave,
        csrc/ctc_align_hip.hip). ``logits_list`` is what align_batch takes; ``texts[u]`` (character alphabets) is a list of
        str, ``tokens[u]`` a list of lists of label ids, the only form for BPE alphabets. An occurrence is a window of frames
        that begins on the phrase's first label and ends on its last, scored by its best CTC path; per end frame the best
        window is kept. Up to ``max_hits`` (1 .. 64) pairwise disjoint windows are taken, best first, none below ``min_logp``
        (None: no threshold); an end frame whose best window overlaps a hit already taken is dropped, even if a worse window
        ending there would not overlap. ``trace=True`` also returns the per-frame ``end_logp`` / ``end_start``."""
        if isinstance(logits_list, (_ResidentBeams, _DeviceStreams)) or (
                isinstance(logits_list, (list, tuple)) and any(isinstance(x, (_ResidentBeams, _DeviceStreams)) for x in logits_list)):
            raise NotImplementedError("find_batch searches utterances' matrices; the frames a stream has consumed are not kept")
        logits_list, phrases = self._many_targets_each("find", "phrase", "phrases", logits_list, texts, tokens)
        for u, cur in enumerate(phrases):
            for j, ids in enumerate(cur):
                if not ids:
                    raise ValueError("find: utterance %d, phrase %d is empty: it would occur everywhere and nowhere" % (u, j))
        if isinstance(max_hits, bool) or not isinstance(max_hits, (int, np.integer)) or not 1 <= int(max_hits) <= FIND_MAX_HITS:
            raise ValueError("find: max_hits must be an int in 1 .. %d, not %r" % (FIND_MAX_HITS, max_hits))
        floor = -math.inf if min_logp is None else float(min_logp)
        if math.isnan(floor):
            raise ValueError("find: min_logp is not a number")
        n = len(phrases)
        self.last_find_timing_ms, self.last_find_launches, self.last_find_launched = (0.0, 0.0, 0.0, 0.0), 0, (0, 0)
        if n == 0:
            return []
        kernel = _forced_kernel("CTCDEC_FIND_KERNEL", FIND_KERNELS)
        with self._call_lock:
            batch, frames, ptrs, c_utts = self._stage_transcript_call(logits_list)
            budget = int(_trace_budget) or ALIGN_BP_BUDGET
            for u, cur in enumerate(phrases):
                for j, ids in enumerate(cur):
                    if int(frames[u]) >= self._frames_needed(ids) and 12 * int(frames[u]) > budget:
                        raise ValueError("find: utterance %d, phrase %d needs a trace of %d bytes, above the memory budget of %d "
                                         "bytes of one launch" % (u, j, 12 * int(frames[u]), budget))
            flat, label_off, hyp_off, n_phrases = self._pack_items(phrases)
            res = C.c_void_p()
            lib = self._lib
            lib.check(lib.dll.ctcdec_find_batch(
                self._handle, *c_utts, n,
                batch.dtype, int(batch.is_device), B.off_ptr(hyp_off), B.off_ptr(label_off), flat.ctypes.data_as(C.POINTER(C.c_int32)),
                int(max_hits), floor, int(bool(trace)), kernel, int(_trace_budget), C.byref(res)))
            try:
                ho, ps, pe, pl, nph = (C.POINTER(C.c_int64)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(),
                                       C.POINTER(C.c_double)(), C.c_int64())
                lib.check(lib.dll.ctcdec_search_hits(res, C.byref(ho), C.byref(ps), C.byref(pe), C.byref(pl), C.byref(nph)))
                if int(nph.value) != n_phrases:
                    raise B.NativeError("the search holds another number of phrases than was asked for")
                hit_off = np.ctypeslib.as_array(ho, shape=(n_phrases + 1,)).tolist()
                nh = hit_off[-1]
                starts = np.ctypeslib.as_array(ps, shape=(nh,)).tolist() if nh else []
                ends = np.ctypeslib.as_array(pe, shape=(nh,)).tolist() if nh else []
                logps = np.ctypeslib.as_array(pl, shape=(nh,)).tolist() if nh else []
                t_off, t_logp, t_start = None, None, None
                if trace:
                    to, tl, ts = C.POINTER(C.c_int64)(), C.POINTER(C.c_double)(), C.POINTER(C.c_int32)()
                    lib.check(lib.dll.ctcdec_search_trace(res, C.byref(to), C.byref(tl), C.byref(ts)))
                    t_off = np.ctypeslib.as_array(to, shape=(n_phrases + 1,)).tolist()
                    nt = t_off[-1]
                    t_logp = np.ctypeslib.as_array(tl, shape=(nt,)).copy() if nt else np.zeros(0)
                    t_start = np.ctypeslib.as_array(ts, shape=(nt,)).copy() if nt else np.zeros(0, dtype=np.int32)
                ms, launches, launched = (C.c_double * 4)(), C.c_int32(), (C.c_int64 * 2)()
                lib.dll.ctcdec_search_timing(res, ms, C.byref(launches), launched)
                # [classification (frame-prune kernels), row_lse, find kernels (HIP events), whole native call]; kernel launches
                # made; phrases that went to (ctc_find_wave, ctc_find)
                self.last_find_timing_ms = tuple(float(v) for v in ms)
                self.last_find_launches = int(launches.value)
                self.last_find_launched = (int(launched[0]), int(launched[1]))
            finally:
                lib.dll.ctcdec_search_free(res)
        out: List[List[PhraseSearch]] = []
        h = 0
        for cur in phrases:
            found = []
            for ids in cur:
                hits = [PhraseHit(starts[k], ends[k], logps[k]) for k in range(hit_off[h], hit_off[h + 1])]
                el = es = None
                if trace:
                    el, es = t_logp[t_off[h]:t_off[h + 1]].copy(), t_start[t_off[h]:t_off[h + 1]].copy()
                found.append(PhraseSearch(self._words_of_target(ids)[0], list(ids), hits, el, es))
                h += 1
            out.append(found)
        return out

    # -- frame posteriors (no reference analogue; DESIGN.md, "Frame posteriors") ---------------------------
    def posteriors(self, logits: Any, text: Optional[str] = None, tokens: Optional[Sequence[int]] = None,
                   dense: bool = True) -> "TranscriptPosteriors":
        """The frame posteriors of one utterance's transcript: posteriors_batch of a batch of one (a ValueError when no
        alignment exists)."""
        self._check_logits_dimension(logits)
        return self.posteriors_batch([logits], None if text is None else [text], tokens=None if tokens is None else [tokens],
                                     dense=dense)[0]

    def posteriors_batch(self, logits_list: Any, texts: Optional[Sequence[str]] = None,
                         tokens: Optional[Sequence[Sequence[int]]] = None, dense: bool = True, strict: bool = True,
                         _table_budget: int = 0) -> List[Optional["TranscriptPosteriors"]]:
        """Under all alignments of each known transcript, where its frames lie, in one native call: per utterance the CTC
        forward-backward for its target (row_lse + ctc_posteriors, csrc/ctc_align_hip.hip), as TranscriptPosteriors. The
        arguments are align_batch's: ``logits_list``, ``texts`` or ``tokens`` (the only form for BPE alphabets), and
        ``strict`` for utterances with fewer frames than target labels plus adjacent equal labels, which have no alignment.
        ``dense=True`` returns every utterance's ``gamma`` as a host array of ``8 * T * (2 L + 1)`` bytes, copied launch by
        launch -- 26 GB for 4096 utterances of 1000 frames and 100 labels: a large batch wants ``dense=False``, which returns
        the scores and the per-token ``occupancy`` / ``centre`` alone, with the same bits."""
        logits_list, targets = self._one_target_each("posteriors", logits_list, texts, tokens)
        n = len(targets)
        self.last_posteriors_timing_ms, self.last_posteriors_launches, self.last_posteriors_launched = (0.0,) * 4, 0, (0, 0)
        if n == 0:
            return []
        with self._call_lock:
            batch, frames, ptrs, _ = self._stage_transcript_call(logits_list)
            keep = self._feasible("posteriors", frames, targets, self._state_table_bytes, int(_table_budget) or POSTERIORS_TABLE_BUDGET, strict)
            out: List[Optional[TranscriptPosteriors]] = [None] * n
            if not keep:
                return out
            k_ptrs = np.ascontiguousarray(ptrs[keep])
            k_frames = np.ascontiguousarray(frames[keep])
            flat, off = self._pack_ids([targets[u] for u in keep])
            res = C.c_void_p()
            lib = self._lib
            lib.check(lib.dll.ctcdec_posteriors_batch(
                self._handle, *self._c_utts(k_ptrs, k_frames),
                len(keep), batch.dtype, int(batch.is_device), B.off_ptr(off), flat.ctypes.data_as(C.POINTER(C.c_int32)),
                int(bool(dense)), int(_table_budget), C.byref(res)))
            try:
                pl, pb, nu = C.POINTER(C.c_double)(), C.POINTER(C.c_double)(), C.c_int64()
                lib.check(lib.dll.ctcdec_posteriors_scores(res, C.byref(pl), C.byref(pb), C.byref(nu)))
                to, po, pc, nt = C.POINTER(C.c_int64)(), C.POINTER(C.c_double)(), C.POINTER(C.c_double)(), C.c_int64()
                lib.check(lib.dll.ctcdec_posteriors_tokens(res, C.byref(to), C.byref(po), C.byref(pc), C.byref(nt)))
                go, gs, gp = C.POINTER(C.c_int64)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_double)()
                lib.check(lib.dll.ctcdec_posteriors_gamma(res, C.byref(go), C.byref(gs), C.byref(gp)))
                if int(nu.value) != len(keep) or int(nt.value) != int(off[-1]):
                    raise B.NativeError("the posteriors hold another number of utterances or tokens than was asked for")
                logp = np.ctypeslib.as_array(pl, shape=(len(keep),)).tolist()
                logp_b = np.ctypeslib.as_array(pb, shape=(len(keep),)).tolist()
                ntok = int(nt.value)
                occ = np.ctypeslib.as_array(po, shape=(ntok,)).copy() if ntok else np.zeros(0)
                cen = np.ctypeslib.as_array(pc, shape=(ntok,)).copy() if ntok else np.zeros(0)
                gammas: List[Optional[np.ndarray]] = [None] * len(keep)
                if dense:
                    g_off = np.ctypeslib.as_array(go, shape=(len(keep) + 1,)).tolist()
                    stride = np.ctypeslib.as_array(gs, shape=(len(keep),)).tolist()
                    flat_g = np.ctypeslib.as_array(gp, shape=(g_off[-1],)) if g_off[-1] else np.zeros(0)
                    for j, u in enumerate(keep):
                        T, S = int(frames[u]), 2 * len(targets[u]) + 1
                        gammas[j] = flat_g[g_off[j]:g_off[j + 1]].reshape(T, stride[j])[:, :S].copy()
                ms, launches, launched = (C.c_double * 4)(), C.c_int32(), (C.c_int64 * 2)()
                lib.dll.ctcdec_posteriors_timing(res, ms, C.byref(launches), launched)
                # [classification (frame-prune kernels), row_lse, ctc_posteriors (HIP events), whole native call]; kernel
                # launches made; utterances that went to (the 256-thread kernel, the 1024-thread kernel)
                self.last_posteriors_timing_ms = tuple(float(v) for v in ms)
                self.last_posteriors_launches = int(launches.value)
                self.last_posteriors_launched = (int(launched[0]), int(launched[1]))
            finally:
                lib.dll.ctcdec_posteriors_free(res)
            for j, u in enumerate(keep):
                ids, o = targets[u], int(off[j])
                out[u] = TranscriptPosteriors(self._words_of_target(ids)[0], list(ids), float(logp[j]), float(logp_b[j]), gammas[j],
                                              occ[o:o + len(ids)].copy(), cen[o:o + len(ids)].copy())
            return out

    # -- transcript gradient (no reference analogue; DESIGN.md, "Transcript gradient") ---------------------
    def gradient(self, logits: Any, text: Optional[str] = None, tokens: Optional[Sequence[int]] = None) -> "TranscriptGradient":
        """The gradient of one utterance's transcript likelihood: gradient_batch of a batch of one (a ValueError when no
        alignment exists)."""
        self._check_logits_dimension(logits)
        return self.gradient_batch([logits], None if text is None else [text], tokens=None if tokens is None else [tokens])[0]

    def gradient_batch(self, logits_list: Any, texts: Optional[Sequence[str]] = None,
                       tokens: Optional[Sequence[Sequence[int]]] = None, strict: bool = True,
                       _table_budget: int = 0) -> List[Optional["TranscriptGradient"]]:
        """The derivative of each known transcript's CTC likelihood with respect to its utterance's matrix, in one native
        call: row_lse, a dense ctc_posteriors launch and ctc_grad_rows over its tables (csrc/ctc_align_hip.hip), as
        TranscriptGradient. Arguments, checks and limits are posteriors_batch's. Host arrays give numpy arrays; device
        tensors give torch tensors on the same device -- views of one allocation the kernel writes in place, never copied to
        the host."""
        return self._gradient_batch(logits_list, texts, tokens, strict, _table_budget)[0]

    def _gradient_batch(self, logits_list, texts, tokens, strict, _table_budget):
        """-> (gradient_batch's list, the one buffer every ``grad`` is a view of -- None without rows --, the utterances that
        have an alignment)."""
        logits_list, targets = self._one_target_each("gradient", logits_list, texts, tokens)
        n, n_labels = len(targets), len(self._labels_list)
        self.last_gradient_timing_ms, self.last_gradient_launches, self.last_gradient_launched = (0.0,) * 5, 0, (0, 0)
        if n == 0:
            return [], None, []
        with self._call_lock:
            batch, frames, ptrs, _ = self._stage_transcript_call(logits_list)
            keep = self._feasible("gradient", frames, targets, self._state_table_bytes, int(_table_budget) or POSTERIORS_TABLE_BUDGET, strict)
            out: List[Optional[TranscriptGradient]] = [None] * n
            if not keep:
                return out, None, keep
            k_ptrs = np.ascontiguousarray(ptrs[keep])
            k_frames = np.ascontiguousarray(frames[keep])
            flat, off = self._pack_ids([targets[u] for u in keep])
            # one buffer for every utterance's rows, of float64 for float64 input and float32 otherwise: the shell makes it,
            # the native call fills it -- on the device for device tensors
            row0 = np.zeros(len(keep) + 1, dtype=np.int64)
            row0[1:] = np.cumsum(k_frames, dtype=np.int64)
            wide = batch.dtype == 1
            if batch.is_device:
                import torch

                buf = torch.empty(int(row0[-1]) * n_labels, dtype=torch.float64 if wide else torch.float32, device=batch.keep[0].device)
                base, size = buf.data_ptr(), buf.element_size()
            else:
                buf = np.empty(int(row0[-1]) * n_labels, dtype=np.float64 if wide else np.float32)
                base, size = buf.ctypes.data, buf.itemsize
            g_ptrs = (np.uint64(base) + row0[:-1].astype(np.uint64) * np.uint64(n_labels * size)).astype(np.uint64)
            logp = np.zeros(len(keep), dtype=np.float64)
            ms, launches, launched = (C.c_double * 5)(), C.c_int32(), (C.c_int64 * 2)()
            lib = self._lib
            lib.check(lib.dll.ctcdec_gradient_batch(
                self._handle, *self._c_utts(k_ptrs, k_frames),
                len(keep), batch.dtype, int(batch.is_device), B.off_ptr(off), flat.ctypes.data_as(C.POINTER(C.c_int32)),
                g_ptrs.ctypes.data_as(C.POINTER(C.c_void_p)), 1 if wide else 0, int(_table_budget),
                logp.ctypes.data_as(C.POINTER(C.c_double)), ms, C.byref(launches), launched))
            # [classification (frame-prune kernels), row_lse, ctc_posteriors, ctc_grad_rows (HIP events), whole native call];
            # kernel launches made (both kernels); utterances that went to (the 256-thread, the 1024-thread) ctc_posteriors
            self.last_gradient_timing_ms = tuple(float(v) for v in ms)
            self.last_gradient_launches = int(launches.value)
            self.last_gradient_launched = (int(launched[0]), int(launched[1]))
            for j, u in enumerate(keep):
                ids = targets[u]
                grad = buf[int(row0[j]) * n_labels:int(row0[j + 1]) * n_labels].reshape(int(k_frames[j]), n_labels)
                out[u] = TranscriptGradient(self._words_of_target(ids)[0], list(ids), float(logp[j]), grad)
            return out, buf, keep

    def ctc_loss(self, logits: Any, texts: Optional[Sequence[str]] = None, tokens: Optional[Sequence[Sequence[int]]] = None,
                 reduction: str = "sum"):
        """``-logp`` of each utterance's transcript as a differentiable torch value: ``logits`` is a list of ``[T, V]`` device
        tensors or one ``[B, T, V]`` device tensor, ``texts`` / ``tokens`` gradient_batch's. Returns a float64 tensor of B
        values (``reduction="none"``) or their sum (``"sum"``), the floats of ``-score``. The forward pass makes one native
        call and keeps its gradient; ``backward`` hands ``-grad * grad_output`` to each input, in its dtype and shape. There is
        no ``"mean"``: torch's divides by the target lengths, other libraries by the batch size -- divide the result by what
        the training recipe means. An utterance without an alignment raises a ValueError."""
        import torch

        if reduction not in ("sum", "none"):
            raise ValueError("ctc_loss: reduction is 'sum' or 'none' (divide by what the recipe calls the mean), not %r" % (reduction,))
        cube = getattr(logits, "ndim", 0) == 3
        xs = [logits] if cube else list(logits)
        if not all(isinstance(x, torch.Tensor) and x.is_cuda for x in xs):
            raise ValueError("ctc_loss: the logits are device tensors (gradient_batch takes host arrays)")
        return _ctc_loss_function().apply(self, texts, tokens, reduction, cube, *xs)

    # -- serialisation (decoder.py:947-1043): alphabet.json + language_model/ --------------------------
    _ALPHABET_SERIALIZED_FILENAME = "alphabet.json"
    _LANGUAGE_MODEL_SERIALIZED_DIRECTORY = "language_model"

    def save_to_dir(self, filepath: str) -> None:
        """Layout of decoder.py:947-962: <dir>/alphabet.json and, with a language model, <dir>/language_model/."""
        alphabet_file = os.path.join(filepath, self._ALPHABET_SERIALIZED_FILENAME)
        with open(alphabet_file, "w") as out:
            out.write(self._alphabet.dumps())
        if self._language_model is None:
            logger.info("decoder has no language model.")
            return
        lm_dir = os.path.join(filepath, self._LANGUAGE_MODEL_SERIALIZED_DIRECTORY)
        os.makedirs(lm_dir)
        logger.info("Saving language model to %s", lm_dir)
        self._language_model.save_to_dir(lm_dir)

    @staticmethod
    def parse_directory_contents(filepath: str) -> Dict[str, Optional[str]]:
        """Where the parts of a saved decoder are (decoder.py:964-990): {"alphabet": path, "language_model": dir or None}.
        Hidden and dunder entries are ignored; anything else besides the two known names is an error."""
        alphabet_name = BeamSearchDecoderCTC._ALPHABET_SERIALIZED_FILENAME
        lm_name = BeamSearchDecoderCTC._LANGUAGE_MODEL_SERIALIZED_DIRECTORY
        entries = sorted(e for e in os.listdir(filepath) if not e.startswith((".", "__")))
        if alphabet_name not in entries:
            raise ValueError(f"Could not find alphabet file {alphabet_name}. Found {entries}")
        others = [e for e in entries if e != alphabet_name]
        if others and lm_name not in others:
            raise ValueError(f"Could not find language model directory. Looking for {lm_name}, found {others}")
        return {"alphabet": os.path.join(filepath, alphabet_name),
                "language_model": os.path.join(filepath, lm_name) if others else None}

    @classmethod
    def load_from_dir(cls, filepath: str, unigram_encoding: Optional[str] = None) -> "BeamSearchDecoderCTC":
        """Inverse of save_to_dir (decoder.py:992-1005)."""
        parts = cls.parse_directory_contents(filepath)
        with open(parts["alphabet"]) as src:
            alphabet = Alphabet.loads(src.read())
        lm_dir = parts["language_model"]
        lm = None if lm_dir is None else LanguageModel.load_from_dir(lm_dir, unigram_encoding=unigram_encoding)
        return cls(alphabet, language_model=lm)

    @classmethod
    def load_from_hf_hub(cls, model_id: str, cache_dir: Optional[str] = None, **kwargs: Any) -> "BeamSearchDecoderCTC":
        """decoder.py:1007-1043: fetch a saved decoder directory from the Hugging Face hub (default cache
        ~/.cache/pyctcdecode) and load it."""
        try:
            import huggingface_hub
        except ImportError as exc:
            raise ImportError("load_from_hf_hub needs the huggingface_hub package "
                              "(https://pypi.org/project/huggingface-hub/).") from exc
        if cache_dir is None:
            cache_dir = os.path.join(os.path.expanduser("~"), ".cache", "pyctcdecode")
        return cls.load_from_dir(huggingface_hub.snapshot_download(model_id, cache_dir=cache_dir, **kwargs))

    # -- streaming (decoder.py:669-728) ----------------------------------------------------------
    def get_starting_state(self):
        """decoder.py:669-679: (beams, cached_lm_scores, cached_p_lm_scores) to start a stream with."""
        start_beam = [EMPTY_START_BEAM]
        language_model = self._language_model
        if language_model is None:
            cached_lm_scores: Dict[Any, Any] = {}
        else:
            # (a dict -- with the reference's one starting entry -- that files what device reads return lazily: _LazyMemo)
            cached_lm_scores = _LazyMemo({("", False): (0.0, 0.0, language_model.get_start_state())})
        cached_p_lm_scores: Dict[str, float] = {}
        return start_beam, cached_lm_scores, cached_p_lm_scores

    def _memo_entry(self, cached_lm_scores, text: str):
        """(raw LM score, KenlmState) of a completed-words text; the device returns these for every beam it
        hands out, so a miss only happens for beams the caller built by hand (scored word by word here)."""
        hit = cached_lm_scores.get((text, False))
        if hit is not None:
            return hit[1], hit[2]
        lm = self._language_model
        if ("", False) not in cached_lm_scores:
            cached_lm_scores[("", False)] = (0.0, 0.0, lm.get_start_state())
        _, raw, state = cached_lm_scores[("", False)]
        so_far = ""
        for word in text.split():
            so_far = word if not so_far else so_far + " " + word
            nxt = cached_lm_scores.get((so_far, False))
            if nxt is None:
                score, st = lm.score(state, word)
                nxt = (raw + score, raw + score, st)
                cached_lm_scores[(so_far, False)] = nxt
            _, raw, state = nxt
        return raw, state

    def partial_decode_beams_batch(
        self,
        logits_list: Sequence[Any],
        cached_lm_scores_list: Sequence[Dict[Any, Any]],
        cached_p_lm_scores_list: Sequence[Dict[str, float]],
        beams_list: Sequence[List[Beam]],
        processed_frames_list: Sequence[int],
        beam_width: int = DEFAULT_BEAM_WIDTH,
        beam_prune_logp: float = DEFAULT_PRUNE_LOGP,
        token_min_logp: float = DEFAULT_MIN_TOKEN_LOGP,
        prune_history: bool = DEFAULT_PRUNE_BEAMS,
        hotword_scorer: Optional[HotwordScorer] = None,
        force_next_word: bool = False,
        is_end: bool = False,
        token_frames: bool = False,
        confidence: Optional[str] = None,
    ) -> List[List[LMBeam]]:
        """Many independent streams advanced by one chunk each in ONE device launch (extension of
        partial_decode_beams, decoder.py:681-728).

        token_frames=True: the beams are TokenLMBeams, with the tokens of the stream so far; confidence="mean" | "min" | "max":
        ConfidenceLMBeams, with per-token and per-word confidences as decode_beams(confidence=...) gives them. Both need the
        stream to be device-resident from its start -- beams handed back unchanged, the default; lists the caller built or
        edited, a seeded memo, a changed hot-word set or CTCDEC_RESIDENT_STREAMS=0 raise NotImplementedError --, and a
        confidence has to be asked for from the stream's first chunk on, with the same fold and with processed_frames that
        continue the stream (ValueError otherwise).

        The streams are device-resident (ctcdec_stream_*): the beams, their LM states and the words decoded so far stay
        on the GPU between chunks. What comes back is, per stream, a list of LMBeam that fills itself the first time it
        is looked at; handed back unchanged in the next call (the reference's own usage pattern) it never has to, and a
        chunk costs two kernel launches. Lists that are built or edited by the caller -- and everything under
        CTCDEC_RESIDENT_STREAMS=0 -- go the reference's way: the host resolves every beam's strings for the device.
        One caveat of the lazy lists: beams that were handed back can only be read until that next call returns its
        own (the device state has moved on); read them first, or keep ``list(beams)``."""
        with self._call_lock:
            return self._partial_decode_beams_batch_locked(
                logits_list, cached_lm_scores_list, cached_p_lm_scores_list, beams_list, processed_frames_list,
                beam_width, beam_prune_logp, token_min_logp, prune_history, hotword_scorer, force_next_word, is_end,
                token_frames, confidence)

    def _partial_decode_beams_batch_locked(
        self, logits_list, cached_lm_scores_list, cached_p_lm_scores_list, beams_list, processed_frames_list,
        beam_width, beam_prune_logp, token_min_logp, prune_history, hotword_scorer, force_next_word, is_end,
        token_frames=False, confidence=None,
    ) -> List[List[LMBeam]]:
        token_mode = _confidence_fold(confidence) or int(bool(token_frames))
        n = len(logits_list)
        if n == 0:
            return []
        for logits in logits_list:
            self._check_logits_dimension(logits)
        hot_sets = None
        if isinstance(hotword_scorer, (list, tuple)):  # one scorer (or None) per stream
            if len(hotword_scorer) != n:
                raise ValueError("hotword_scorer holds %d per-stream entries for %d streams" % (len(hotword_scorer), n))
            if any(h is not None and not isinstance(h, HotwordScorer) for h in hotword_scorer):
                raise TypeError("hotword_scorer entries must be None or pyctcdecode_amd HotwordScorers")
            hot_sets = _per_utt_hot([h.unigrams if h is not None else None for h in hotword_scorer],
                                    [h.weight if h is not None else 0.0 for h in hotword_scorer], n, normalise=False)
            sets, utt_set = hot_sets
            if all(k == utt_set[0] for k in utt_set):  # one set for every stream: the call-wide way
                hot_sets = None
                hotword_scorer = HotwordScorer(list(sets[utt_set[0]][0]), sets[utt_set[0]][1]) if utt_set[0] >= 0 else None
        if hotword_scorer is not None and hot_sets is None and not isinstance(hotword_scorer, HotwordScorer):
            raise TypeError("hotword_scorer must be a pyctcdecode_amd HotwordScorer")
        weight = hotword_scorer.weight if hotword_scorer is not None and hot_sets is None else 0.0
        unigrams = hotword_scorer.unigrams if hotword_scorer is not None and hot_sets is None else []
        # (the carried beams' view of their open word depends on the words: another list means importing them again)
        key = tuple(unigrams) if hot_sets is None else ("per-stream",) + tuple(
            hot_sets[0][k][0] if k >= 0 else () for k in hot_sets[1])
        for beams in beams_list:
            if not isinstance(beams, _ResidentBeams) and len(beams) == 0:
                raise ValueError("a stream needs at least one beam (use get_starting_state())")
        params = self._params(beam_width, beam_prune_logp, token_min_logp, prune_history, weight, 0)
        # refused here, before any stream is opened, imported into or retired: the lists of the previous chunk stay readable
        # (the library refuses the same values with the same exceptions, api.cpp: check_call)
        if params.beam_width < 1:
            raise ValueError("beam_width must be >= 1")
        if params.beam_width > B.MAX_BEAM_WIDTH:
            raise NotImplementedError("beam_width above the supported maximum of %d" % B.MAX_BEAM_WIDTH)
        lazy_ok = os.environ.get("CTCDEC_RESIDENT_STREAMS", "1") != "0"
        # which device streams do these beams belong to?
        streams: Optional[_DeviceStreams] = None
        first = beams_list[0]
        handed_back = (isinstance(first, _ResidentBeams) and first._streams.alive(self) and first._streams.n == n and
                       all(isinstance(b, _ResidentBeams) and b._streams is first._streams and b._index == u and b._current()
                           for u, b in enumerate(beams_list)))
        resident = handed_back and first._streams.hot_key == key
        at_start = not resident and all(len(b) == 1 and b[0] == EMPTY_START_BEAM for b in beams_list)
        fresh = at_start and all(self._memo_starts_at_default(m) for m in cached_lm_scores_list)
        frames_in = [int(p) for p in processed_frames_list]
        if token_mode or (resident and first._streams.token_mode > 1):
            # tokens and confidences come from the chains and the survivor ledger of a stream that has been on the device from
            # its start: every other route is refused here, before any stream is opened, imported into or retired
            self._check_stream_tokens(token_mode, lazy_ok, handed_back, resident, at_start, fresh,
                                      first._streams if resident else None, frames_in)
        if hot_sets is None and key != self._hot_key:
            blob, off = B.pack_strings(unigrams)
            self._lib.check(self._lib.dll.ctcdec_set_hotwords(self._handle, blob, B.off_ptr(off), len(unigrams)))
            self._hot_key = key
        if resident:
            streams = first._streams  # handed back unchanged: nothing to import
        elif fresh:
            streams = _DeviceStreams(self, n)  # the reference's starting state: the model's own start state, nothing scored
        else:
            # built or edited by the caller (or fed to another call in between): the host resolves their strings
            streams = _DeviceStreams(self, n)
            streams.import_beams(beams_list, cached_lm_scores_list, hot_sets)
        streams.hot_key = key
        streams.hot_sets = hot_sets
        batch = _Batch(logits_list, len(self._idx2vocab))
        if batch.is_device and batch.device_index is not None and batch.device_index != self._device:
            raise ValueError("the logits live on cuda:%d but this decoder was built for cuda:%d (one process per GPU: "
                             "LOCAL_RANK / CTCDEC_DEVICE pick the device)" % (batch.device_index, self._device))
        ptrs, frames = _c_arrays(batch)
        first_frames = (C.c_int32 * n)(*frames_in)
        want = bool(is_end) or not lazy_ok
        res = C.c_void_p()
        params.token_frames = token_mode
        streams.retire_lists()
        if hot_sets is not None:
            self._arm_hot_sets(hot_sets)
        self._lib.check(self._lib.dll.ctcdec_stream_push(
            streams.handle, ptrs, frames, batch.dtype, int(batch.is_device), C.byref(params), first_frames,
            int(bool(force_next_word)), int(bool(is_end)), int(want), C.byref(res)))
        streams.params = params
        streams.memos = list(cached_lm_scores_list)
        if is_end:
            streams.token_mode, streams.next_frame = 0, None
        else:
            if streams.next_frame is None:
                streams.token_mode = token_mode
            streams.next_frame = [f + int(t) for f, t in zip(frames_in, batch.frames)]
        try:
            if want:
                return streams.unpack(res)
        finally:
            if res:
                self._lib.dll.ctcdec_result_free(res)
        return streams.lazy_lists()

    @staticmethod
    def _check_stream_tokens(token_mode: int, lazy_ok: bool, handed_back: bool, resident: bool, at_start: bool, fresh: bool,
                             streams: Optional[_DeviceStreams], frames_in: List[int]) -> None:
        """partial_decode_beams(token_frames=... / confidence=...): the routes that cannot serve them, and a stream's fold and
        frame numbering (what the library refuses itself, api.cpp: check_stream_tokens, raised here while the previous
        chunk's lists are still readable)."""
        what = "token_frames / confidence of a streaming decode"
        if not lazy_ok:
            raise NotImplementedError(what + " need device-resident streams, which CTCDEC_RESIDENT_STREAMS=0 turns off")
        if streams is None:
            if handed_back:
                raise NotImplementedError(what + ": the hot words changed, so the beams are imported again and their chains "
                                                 "no longer reach back to the start of the stream")
            if at_start and not fresh:
                raise NotImplementedError(what + ": cached_lm_scores was seeded with another start state, so the stream "
                                                 "starts from imported beams, whose chains carry no tokens")
            if not at_start:
                raise NotImplementedError(what + " need the beams handed back as partial_decode_beams returned them: lists the "
                                                 "caller built or edited are imported, and their chains carry no tokens")
            return  # a fresh stream: anything goes
        if streams.parents is not None:
            raise NotImplementedError(what + ": this stream was started from imported beams, whose chains carry no tokens")
        fold = streams.token_mode if streams.token_mode > 1 else 0
        if token_mode > 1 and token_mode != fold:
            raise ValueError("confidence has to be asked for from a stream's first chunk on, with the same fold every time"
                             if not fold else "a stream keeps the confidence fold its first chunk asked for")
        if fold and streams.next_frame is not None and frames_in != streams.next_frame:
            raise ValueError("processed_frames %r does not continue the stream (confidence: expected %r)"
                             % (frames_in, streams.next_frame))

    def _memo_starts_at_default(self, memo: Dict[Any, Any]) -> bool:
        """Is the memo's entry for the empty text what get_starting_state() puts there -- (0, 0, the model's start state)?
        The reference scores a stream's first word from THAT entry's state (decoder.py:387-396): a caller that seeds it with
        the last_lm_state of a previous segment must not be decoded from the beginning of a sentence (such streams take the
        import path, which reads the entry)."""
        lm = self._language_model
        if lm is None:
            return True
        entry = memo.get(("", False)) if hasattr(memo, "get") else None
        if entry is None:
            return True
        try:
            lm_hw, raw, state = entry
        except (TypeError, ValueError):
            return False
        return lm_hw == 0.0 and raw == 0.0 and _same_lm_state(state, lm.get_start_state())

    def partial_decode_beams(
        self,
        logits: Any,
        cached_lm_scores: Dict[Any, Any],
        cached_p_lm_scores: Dict[str, float],
        beams: List[Beam],
        processed_frames: int,
        beam_width: int = DEFAULT_BEAM_WIDTH,
        beam_prune_logp: float = DEFAULT_PRUNE_LOGP,
        token_min_logp: float = DEFAULT_MIN_TOKEN_LOGP,
        prune_history: bool = DEFAULT_PRUNE_BEAMS,
        hotword_scorer: Optional[HotwordScorer] = None,
        force_next_word: bool = False,
        is_end: bool = False,
        token_frames: bool = False,
        confidence: Optional[str] = None,
    ) -> List[LMBeam]:
        """decoder.py:681-728: advance one stream by one chunk; feed the returned beams back in.
        token_frames / confidence: TokenLMBeams / ConfidenceLMBeams (partial_decode_beams_batch)."""
        return self.partial_decode_beams_batch(
            [logits], [cached_lm_scores], [cached_p_lm_scores], [beams], [processed_frames], beam_width,
            beam_prune_logp, token_min_logp, prune_history, hotword_scorer, force_next_word, is_end, token_frames, confidence,
        )[0]


def build_ctcdecoder(
    labels: List[str],
    kenlm_model_path: Optional[str] = None,
    unigrams: Optional[Collection[str]] = None,
    alpha: float = DEFAULT_ALPHA,
    beta: float = DEFAULT_BETA,
    unk_score_offset: float = DEFAULT_UNK_LOGP_OFFSET,
    lm_score_boundary: bool = DEFAULT_SCORE_LM_BOUNDARY,
) -> BeamSearchDecoderCTC:
    """decoder.py:1051-1099: alphabet from `labels`; with a model path, an n-gram LanguageModel over it. The unigram list
    of an .arpa file is read from the file itself when none is given; any other model format carries none."""
    from_arpa = kenlm_model_path is not None and kenlm_model_path.endswith(".arpa")
    if from_arpa:
        logger.info("Using arpa instead of binary LM file, decoder instantiation might be slow.")
    model = NgramModel(kenlm_model_path) if kenlm_model_path is not None else None
    if unigrams is None and from_arpa:
        unigrams = load_unigram_set_from_arpa(kenlm_model_path)
    elif unigrams is None and model is not None:
        logger.warning("Unigrams not provided and cannot be automatically determined from LM file (only "
                       "arpa format). Decoding accuracy might be reduced.")
    alphabet = Alphabet.build_alphabet(labels)
    if unigrams is not None:
        verify_alphabet_coverage(alphabet, unigrams)
    if model is None:
        return BeamSearchDecoderCTC(alphabet, None)
    lm = LanguageModel(model, unigrams, alpha=alpha, beta=beta, unk_score_offset=unk_score_offset,
                       score_boundary=lm_score_boundary)
    return BeamSearchDecoderCTC(alphabet, lm)
