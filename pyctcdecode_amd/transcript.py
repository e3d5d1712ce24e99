"""The transcript family of the Python surface: what is known about an utterance's text is given, and the library says
where it lies, how probable it is, or what it asks of the logits -- forced alignment (plain, long, tiled, with gaps),
greedy decoding, transcript likelihood, prefix scores and sessions, phrase search and spotting (on whole utterances and
on streams), frame posteriors and the CTC gradient. None of it has an analogue in the reference. The calls are methods
of ``_TranscriptCalls``, a base class of ``decoder.BeamSearchDecoderCTC``; ``decoder`` imports this module, never the
other way round at import time. All work happens in libctcdec through ctypes; this file only marshals."""
from __future__ import annotations

import ctypes as C
import dataclasses
import itertools
import math
import os
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _binding as B

Frames = Tuple[int, int]
WordFrames = Tuple[str, Frames]


_STREAM_CLASSES: tuple = ()  # decoder's _ResidentBeams and _DeviceStreams, looked up at the first call: decoder imports this module


def _refuse_streams(logits: Any, who: str, does: str, batch: bool = True) -> None:
    """The transcript calls read whole matrices: a handle of a device-resident stream (or, ``batch``, a list that holds
    one) is refused in the call's own words."""
    global _STREAM_CLASSES
    if not _STREAM_CLASSES:
        from .decoder import _DeviceStreams, _ResidentBeams

        _STREAM_CLASSES = (_ResidentBeams, _DeviceStreams)
    streams = _STREAM_CLASSES
    if isinstance(logits, streams) or (batch and isinstance(logits, (list, tuple)) and any(isinstance(x, streams) for x in logits)):
        raise NotImplementedError("%s %s; the frames a stream has consumed are not kept" % (who, does))


def _bounded_int(v: Any, lo: int, top: int, message: str, *args) -> int:
    """``v`` as an int in [lo, top); else a ValueError of ``message % (args + (v,))``. A bool is no int here."""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) < top:
        raise ValueError(message % (args + (v,)))
    return int(v)


def _texts_or_tokens(what: str, texts, tokens):
    """-> whichever of the two was given"""
    if (texts is None) == (tokens is None):
        raise ValueError("%s: give exactly one of texts and tokens" % what)
    return texts if texts is not None else tokens


def _no_text_under_bpe(give: str) -> ValueError:
    return ValueError("a text has many segmentations under a BPE alphabet: give the %s" % give)


ALIGN_MAX_LABELS = 2047  # ALIGN_MAX_LABELS of csrc/ctc_align.h: 2 L + 1 states, two fp64 score columns in a workgroup's LDS
ALIGN_LONG_MAX_LABELS = 1048575  # ALIGN_LONG_MAX_LABELS of csrc/ctc_align.h: 2 L + 1 states below 2^21 (align_long, score_long)
SCORE_LONG_TILE_GROUPS = 256  # FORWARD_TILE_MAX_GROUPS of csrc/ctc_align.h: the groups of four states of a state block, at most
ALIGN_TILED_MAX_SEGMENT = 448  # ALIGN_TILED_MAX_SEGMENT of csrc/ctc_align.h: the frames of a segment whose back-pointers fit LDS, at most
SCORE_LONG_TILE_FRAMES = 64  # FORWARD_TILE_FRAMES of csrc/ctc_align.h: the frames of a time block when there are several state blocks
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
        _refuse_streams(logits_list, "a prefix session", "reads an utterance's matrix at every step")
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
        # [ctc_prefix_advance, ctc_prefix_extend with its finish and fill (HIP events), whole native call]; launches of
        # (ctc_prefix_advance, ctc_prefix_extend / finish / fill, row_lse, the forward kernels)
        self.last_timing_ms, self.last_launches = B.read_out(self._lib, self._lib.dll.ctcdec_prefix_session_timing, self._handle,
                                                             sizes=(3, 4))

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
                raise _no_text_under_bpe("labels")
            labels = []
            for k, t in enumerate(texts):
                if not isinstance(t, str) or len(t) != 1 or t not in dec._vocab2idx:
                    raise ValueError("extend: texts[%d] is %r: not a single character of the alphabet" % (k, t))
                labels.append(dec._vocab2idx[t])
        labels = list(labels)
        if len(labels) != len(parents):
            raise ValueError("extend: %d labels for %d parents" % (len(labels), len(parents)))
        nodes = [self._live("extend", p) for p in parents]
        # (the first error in the order of the children, a child's label before its length)
        long = next((k for k, p in enumerate(nodes) if len(p.tokens) + 1 > ALIGN_MAX_LABELS), len(nodes))
        labels[:long + 1] = dec._label_ids(labels[:long + 1], lambda k: "extend: labels[%d] is" % k)
        if long < len(nodes):
            raise ValueError("extend: child %d has %d labels, above the limit of %d labels per prefix" % (long, len(nodes[long].tokens) + 1, ALIGN_MAX_LABELS))
        n = len(parents)
        if len(self._nodes) + n > self.capacity:
            raise ValueError("extend: %d children, but %d of the session's %d slots are free: release prefixes, or open the session "
                             "with a larger capacity" % (n, self.capacity - len(self._nodes), self.capacity))
        if n == 0:
            return []
        with dec._call_lock:
            buf, next_dev, next_host = self._room(n)
            par = np.ascontiguousarray(parents, dtype=np.int64)
            lab = np.ascontiguousarray(labels, dtype=np.int32)
            ids, end = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.float64)
            self._lib.check(self._lib.dll.ctcdec_prefix_session_extend(
                handle, B.off_ptr(par), lab.ctypes.data_as(C.POINTER(C.c_int32)), n, next_dev, B.off_ptr(ids),
                end.ctypes.data_as(C.POINTER(C.c_double)), next_host))
            self._take_timing()
        return self._nodes_of(ids, [p.utt for p in nodes], [p.tokens + [c] for p, c in zip(nodes, labels)], end, buf)

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


@dataclasses.dataclass(frozen=True)
class SpotHit:
    """One hit of a phrase spotting (BeamSearchDecoderCTC.spot / spot_batch): ``logp`` is the log-probability, summed over
    every alignment, that an occurrence of the phrase ends on frame ``end - 1``; ``start`` is the mass-weighted mean first
    frame of those occurrences, rounded."""

    start: int
    end: int
    logp: float

    @property
    def frames(self) -> int:
        return self.end - self.start

    @property
    def prob(self) -> float:
        return math.exp(self.logp)


@dataclasses.dataclass(frozen=True, eq=False)
class PhraseSpot:
    """How probably a phrase occurs in an utterance (BeamSearchDecoderCTC.spot / spot_batch): ``text`` and ``tokens`` are
    ScoredText's; ``hits`` are the end frames taken, most probable first, their windows pairwise disjoint; ``count`` is the
    expected number of occurrences, the sum over the frames of exp(end_logp) -- 0.0, and no hits, when the utterance has
    fewer frames than the phrase has labels plus adjacent equal labels. With ``trace=True``, ``end_logp[t]`` (float64) is the
    log-probability that an occurrence ends on frame ``t`` and ``end_start[t]`` (int32) the rounded mean first frame of
    those occurrences, ``-inf`` / ``-1`` where none can end; else both are None."""

    text: str
    tokens: List[int]
    hits: List[SpotHit]
    count: float
    end_logp: Optional[np.ndarray] = None
    end_start: Optional[np.ndarray] = None


SPOT_STREAM_MAX_LABELS = 127  # FIND_WAVE_MAX_LABELS of csrc/ctc_align.h: ctc_spot_chunk gives a lane to every four states
SPOT_STREAM_WIDTHS = (8, 16, 32, 64)  # CTCDEC_SPOT_STREAM_WIDTH: the fewest lanes of a wavefront a phrase takes (unset: packed)


@dataclasses.dataclass(frozen=True, eq=False)
class SpotChunk:
    """What one SpotStreams.feed adds to a phrase: the entries of PhraseSpot's trace that became final in this call, frames
    ``first_frame .. first_frame + len(end_logp) - 1`` of the whole stream (``end_start`` counts from the stream's first
    frame too), and ``count``, the expected number of occurrences that end on a frame final so far."""

    text: str
    tokens: List[int]
    first_frame: int
    end_logp: np.ndarray
    end_start: np.ndarray
    count: float


class SpotStreams:
    """Phrase spotting on live streams (BeamSearchDecoderCTC.spot_streams; DESIGN.md, "Phrase spotting on streams"): the
    session keeps every phrase's states on the device, so that ``feed`` advances all phrases of all streams by one chunk each
    in one ctc_spot_chunk launch, and what it returns, chunk after chunk, is float for float the trace spot_batch computes
    from the concatenated chunks. A context manager; ``close()`` frees the device memory."""

    def __init__(self, decoder: "BeamSearchDecoderCTC", texts, tokens, n_streams: Optional[int], max_frames: Optional[int]):
        self._decoder, self._lib, self._handle = decoder, decoder._lib, None
        given = list(_texts_or_tokens("spot_streams", texts, tokens))
        if n_streams is not None:  # one flat list of phrases, shared by every stream
            if isinstance(n_streams, bool) or not isinstance(n_streams, (int, np.integer)) or n_streams < 0:
                raise ValueError("spot_streams: n_streams must be a non-negative int, not %r" % (n_streams,))
            given = [given] * int(n_streams)
        if isinstance(max_frames, bool) or not (max_frames is None or (isinstance(max_frames, (int, np.integer)) and 0 < max_frames < 2 ** 31)):
            raise ValueError("spot_streams: max_frames must be None or an int in 1 .. 2^31 - 1, not %r" % (max_frames,))
        n = len(given)
        placeholder = [np.zeros((0, len(decoder._labels_list)))] * n
        _, phrases = decoder._many_targets_each("spot_streams", "phrase", "phrases", placeholder, given if texts is not None else None,
                                                given if tokens is not None else None)
        for u, cur in enumerate(phrases):
            for j, ids in enumerate(cur):
                if not ids:
                    raise ValueError("spot_streams: stream %d, phrase %d is empty: it would occur everywhere and nowhere" % (u, j))
                if len(ids) > SPOT_STREAM_MAX_LABELS:
                    raise ValueError("spot_streams: stream %d, phrase %d has %d labels, above the limit of %d labels of a phrase "
                                     "spotted on a stream (spot / spot_batch take up to %d on a whole utterance)"
                                     % (u, j, len(ids), SPOT_STREAM_MAX_LABELS, ALIGN_MAX_LABELS))
        self._phrases = phrases
        self._texts = [[decoder._words_of_target(ids)[0] for ids in cur] for cur in phrases]
        self.n_streams, self.max_frames = n, None if max_frames is None else int(max_frames)
        self._fed, self._ended = [0] * n, [False] * n  # frames fed to each stream, and whether it has ended
        flat, label_off, hyp_off, self._n_phrases = decoder._pack_items(phrases)
        handle = C.c_void_p()
        with decoder._call_lock:
            self._lib.check(self._lib.dll.ctcdec_spot_streams_open(
                decoder._handle, n, B.off_ptr(hyp_off), B.off_ptr(label_off), flat.ctypes.data_as(C.POINTER(C.c_int32)),
                self.max_frames or 0, C.byref(handle)))
        self._handle = handle

    def _open_handle(self):
        if self._handle is None:
            raise ValueError("the spotting session is closed")
        return self._handle

    def feed(self, chunks: Any, is_end: Any = False) -> List[List[SpotChunk]]:
        """One chunk ``[frames, V]`` per stream -- host arrays or device tensors of one dtype, 0 frames allowed -- through
        every phrase of its stream; ``is_end`` (a bool, or one per stream) ends a stream with this chunk, after which it
        takes no more frames. Returns per stream, per phrase, a SpotChunk with the entries that became final: entry ``t``
        is final once frame ``t + 1`` has been fed or the stream has ended. Each chunk is told apart as probabilities or
        logits on its own, as a chunk given to partial_decode_beams is. A ValueError leaves the session as it was."""
        handle = self._open_handle()
        dec, n = self._decoder, self.n_streams
        if getattr(chunks, "ndim", 0) != 3:
            chunks = list(chunks)
        if len(chunks) != n:
            raise ValueError("feed: %d chunks for %d streams" % (len(chunks), n))
        ends = [bool(is_end)] * n if isinstance(is_end, (bool, np.bool_)) else [bool(e) for e in is_end]
        if len(ends) != n:
            raise ValueError("feed: %d is_end flags for %d streams" % (len(ends), n))
        width = os.environ.get("CTCDEC_SPOT_STREAM_WIDTH", "")
        if width and width not in [str(w) for w in SPOT_STREAM_WIDTHS]:
            raise ValueError("CTCDEC_SPOT_STREAM_WIDTH must be 8, 16, 32 or 64, not %r" % width)
        lib = self._lib
        with dec._call_lock:
            batch, frames, ptrs, c_utts = dec._stage_transcript_call(chunks)
            for u in range(n):
                if self._ended[u] and int(frames[u]) > 0:
                    raise ValueError("feed: stream %d has ended: it takes no more frames" % u)
                if self.max_frames is not None and self._fed[u] + int(frames[u]) > self.max_frames:
                    raise ValueError("feed: stream %d would hold %d frames, above the session's max_frames of %d"
                                     % (u, self._fed[u] + int(frames[u]), self.max_frames))
            c_end = np.asarray(ends, dtype=np.int32) if n else np.zeros(1, dtype=np.int32)
            eo, ff, el, es, cn = B.read_out(lib, lib.dll.ctcdec_spot_streams_feed, handle, *c_utts, c_end.ctypes.data_as(C.POINTER(C.c_int32)),
                                            batch.dtype, int(batch.is_device), int(width or 0))
            for u in range(n):
                self._fed[u] += int(frames[u])
                self._ended[u] = self._ended[u] or ends[u]
            nph = self._n_phrases
            off = B.values(eo, nph + 1) if nph else [0]
            first, counts = B.values(ff, nph), B.values(cn, nph)
            logp, start = B.values(el, off[-1], copy=True), B.values(es, off[-1], copy=True)
            ms, waves = B.read_out(lib, lib.dll.ctcdec_spot_streams_timing, handle, sizes=(4, 4))
            dec._set_call_stats("spot_stream", ms, 1 if any(waves) else 0, waves)
        out, h = [], 0
        for u, cur in enumerate(self._phrases):
            got = []
            for j, ids in enumerate(cur):
                got.append(SpotChunk(self._texts[u][j], list(ids), first[h], logp[off[h]:off[h + 1]], start[off[h]:off[h + 1]], counts[h]))
                h += 1
            out.append(got)
        return out

    def hits(self, max_hits: int = 1, min_logp: Optional[float] = None) -> List[List[List[SpotHit]]]:
        """spot_batch's hits, per stream and phrase, over the entries final so far: up to ``max_hits`` pairwise disjoint
        windows, most probable end frame first, none below ``min_logp`` (kernel spot_select: find_batch's selection on the
        session's device trace). Needs a session opened with ``max_frames``. Once every stream has ended these are
        spot_batch's hits on the concatenated chunks."""
        handle = self._open_handle()
        if self.max_frames is None:
            raise ValueError("hits: the session keeps no trace to select from: open it with spot_streams(..., max_frames=)")
        max_hits = _bounded_int(max_hits, 1, FIND_MAX_HITS + 1, "hits: max_hits must be an int in 1 .. %d, not %r", FIND_MAX_HITS)
        floor = -math.inf if min_logp is None else float(min_logp)
        if math.isnan(floor):
            raise ValueError("hits: min_logp is not a number")
        lib = self._lib
        with self._decoder._call_lock:
            ho, ps, pe, pl, n = B.read_out(lib, lib.dll.ctcdec_spot_streams_hits, handle, max_hits, floor)
            off = B.values(ho, n + 1) if n else [0]
            starts, ends, logps = B.values(ps, off[-1]), B.values(pe, off[-1]), B.values(pl, off[-1])
        out, h = [], 0
        for cur in self._phrases:
            out.append([[SpotHit(starts[k], ends[k], logps[k]) for k in range(off[h + j], off[h + j + 1])] for j in range(len(cur))])
            h += len(cur)
        return out

    def close(self) -> None:
        if self._handle is not None:
            with self._decoder._call_lock:
                self._lib.dll.ctcdec_spot_streams_close(self._handle)
            self._handle = None

    def __enter__(self) -> "SpotStreams":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 (interpreter shutdown)
            pass


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


class _TranscriptCalls:
    """The transcript calls of BeamSearchDecoderCTC, as its base class. The decoder brings the alphabet (``_alphabet``,
    ``_labels_list``, ``_vocab2idx``, ``_is_bpe``), the library and its handle (``_lib``, ``_handle``, ``_device``), the
    call lock, ``_language_model`` and ``_check_logits_dimension``."""

    def _init_transcript_stats(self) -> None:
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
        # ... and of the last spot / spot_batch call, as find's (the kernels: ctc_spot_wave, ctc_spot)
        self.last_spot_timing_ms = (0.0, 0.0, 0.0, 0.0)
        self.last_spot_launches = 0
        self.last_spot_launched = (0, 0)
        # ... and of the last SpotStreams.feed (ms: classification, row_lse, ctc_spot_chunk, native call; kernel launches made;
        # wavefronts launched with segments of 8, 16, 32 and 64 lanes)
        self.last_spot_stream_timing_ms = (0.0, 0.0, 0.0, 0.0)
        self.last_spot_stream_launches = 0
        self.last_spot_stream_launched = (0, 0, 0, 0)
        # ... and of the last align_gaps / align_gaps_batch call (ms: classification, row_lse_max, ctc_viterbi_gaps, native
        # call; kernel launches made)
        self.last_align_gaps_timing_ms = (0.0, 0.0, 0.0, 0.0)
        self.last_align_gaps_launches = 0
        # ... and of the last align_long / align_long_batch call (ms: classification, row_lse, ctc_viterbi_long, native call;
        # kernel launches made; (segment_frames, n_segments) of every utterance that was aligned)
        self.last_align_long_timing_ms = (0.0, 0.0, 0.0, 0.0)
        self.last_align_long_launches = 0
        self.last_align_long_plan: List[Tuple[int, int]] = []
        self.last_align_tiled_plan: List[Tuple[int, int, int, int, int, int]] = []
        self.last_align_tiled_launches = self.last_align_tiled_tiles = self.last_align_tiled_groups = self.last_align_tiled_widest = 0
        self.last_align_tiled_pass_ms = (0.0, 0.0)
        # ... and of the last score_long / score_long_batch call (ms: classification, row_lse, the fill and ctc_forward_tile's
        # launches, native call; diagonals launched, tiles in them, launch groups; the plan of every hypothesis launched)
        self.last_score_long_timing_ms = (0.0, 0.0, 0.0, 0.0)
        self.last_score_long_launches = self.last_score_long_tiles = self.last_score_long_groups = self.last_score_long_widest = 0
        self.last_score_long_plan: List[Tuple[int, int, int, int, int]] = []
        # ... and of the last align_gaps_long / align_gaps_long_batch call (ms: classification, row_lse_max,
        # ctc_viterbi_gaps_long, native call; launches; plan)
        self.last_align_gaps_long_timing_ms = (0.0, 0.0, 0.0, 0.0)
        self.last_align_gaps_long_launches = 0
        self.last_align_gaps_long_plan: List[Tuple[int, int]] = []
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

    def _token_words(self, ids: Sequence[int], start: Sequence[int], end: Sequence[int], logp: Optional[Sequence[float]], o: int = 0):
        """-> (text, token_frames, text_frames, token_logp, word_logp) of the labels ``ids``, whose frames -- and, unless None,
        confidences -- are entries ``o ..`` of the flat arrays: what AlignedText, GappedAlignment and GreedyText hold."""
        text, kept, words = self._words_of_target(ids)
        labels = self._labels_list
        tok = [(labels[ids[k]], (start[o + k], end[o + k])) for k in kept]
        wf = [(w, (tok[lo][1][0], tok[hi - 1][1][1])) for w, lo, hi in words]
        tlp = wlp = None
        if logp is not None:
            tlp = [logp[o + k] for k in kept]
            wlp = [min(tlp[lo:hi]) for _w, lo, hi in words]
        return text, tok, wf, tlp, wlp

    def _label_ids(self, seq, where, gap: bool = False) -> List[int]:
        """``seq`` as a list of label ids: ints in [0, V) other than the blank, or, with ``gap``, -1. ``where(k)`` opens the
        message about entry k."""
        ids = list(seq)
        n_labels, blank, lo = len(self._labels_list), self._vocab2idx[""], -1 if gap else 0
        if set(map(type, ids)) <= {int} and (not ids or (lo <= min(ids) and max(ids) < n_labels and blank not in ids)):
            return ids  # (plain ints, all in range: the check below, without a Python-level loop)
        for k, c in enumerate(ids):
            if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not lo <= int(c) < n_labels or int(c) == blank:
                raise ValueError("%s %r: not a label id in [0, %d) other than the blank (%d)%s"
                                 % (where(k), c, n_labels, blank, ", nor -1 for a gap" if gap else ""))
            ids[k] = int(c)
        return ids

    def _targets_given(self, what: str, logits_list: Any, texts, tokens, items: Optional[str] = None):
        """-> (logits_list, what was given, one entry per utterance): the checks every transcript call makes of its
        arguments before anything is staged -- texts (character alphabets) or tokens, as many entries as utterances. The
        three front ends (_one_target_each, _gapped_targets, _many_targets_each) then read each entry: one target, or, with
        ``items`` (their plural: "hypotheses"), any iterable of them."""
        given = _texts_or_tokens(what, texts, tokens)
        if texts is not None and self._is_bpe:
            raise _no_text_under_bpe("%s as tokens=" % (items or "target"))
        if getattr(logits_list, "ndim", 0) != 3:
            logits_list = list(logits_list)
        n = len(logits_list)
        if items and not isinstance(given, str):
            given = list(given)  # (a generator has no len())
        if isinstance(given, str) or len(given) != n:
            got = 1 if isinstance(given, str) else len(given)
            if items:
                raise ValueError("%s: %s for %d utterances, but %d utterances" % (what, items, got, n))
            raise ValueError("%s: %d targets for %d utterances" % (what, got, n))
        return logits_list, given

    def _one_target_each(self, what: str, logits_list: Any, texts, tokens, max_labels: int = ALIGN_MAX_LABELS):
        """-> (logits_list, targets): one target per utterance, as a text or as label ids, of at most ``max_labels``."""
        logits_list, given = self._targets_given(what, logits_list, texts, tokens)
        targets: List[List[int]] = []
        for u, g in enumerate(given):
            if texts is not None:
                if not isinstance(g, str):
                    raise ValueError("%s: texts[%d] is not a str" % (what, u))
                ids = self._target_of_text(g)
            else:
                ids = self._label_ids(g, lambda _k: "%s: tokens[%d] holds" % (what, u))
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

    def _keep_feasible(self, what: str, frames: np.ndarray, ptrs: np.ndarray, targets: Sequence[Sequence[int]], table_bytes, budget: int,
                       strict: bool, table_name: str = "table", path_name: str = "alignment", gaps: bool = False):
        """-> (keep, their frame counts, their _c_utts, their targets packed (flat, off)): the staged utterances cut down to
        those that have a path for their labels (``gaps``: a -1 among them is no label); the last four are None when none
        has. One whose table, of ``table_bytes(frames, labels)`` bytes, is above the budget of a launch is a ValueError, and
        so are, when ``strict``, the utterances without a path. The messages call the table and the path by the call's own
        words."""
        keep, bad = [], []
        for u, ids in enumerate(targets):
            if gaps:
                ids = [c for c in ids if c != -1]
            (keep if int(frames[u]) >= self._frames_needed(ids) else bad).append(u)
            table = table_bytes(int(frames[u]), len(ids))
            if table > budget:
                raise ValueError("%s: utterance %d needs a %s of %d bytes, above the memory budget of %d bytes of one launch"
                                 % (what, u, table_name, table, budget))
        if bad and strict:
            raise ValueError("%s: no %s for utterances %s: fewer frames than target labels plus adjacent equal labels"
                             % (what, path_name, bad))
        if not keep:
            return keep, None, None, None, None
        k_frames = np.ascontiguousarray(frames[keep])
        flat, off = self._pack_ids([targets[u] for u in keep])
        return keep, k_frames, self._c_utts(np.ascontiguousarray(ptrs[keep]), k_frames), flat, off

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
                       segment_frames: Optional[int], tiles: Optional[Tuple[int, int, int]] = None):
        """-> (the AlignedText of every utterance, None for one without a path; the stats of the native call, None when none
        was made): the checked targets through _alignment_call, and the words formed from the result."""
        out: List[Optional[AlignedText]] = [None] * len(targets)
        got = self._alignment_call(what, logits_list, targets, fold, strict, bp_budget, segment_frames, tiles)
        if got is None:
            return out, None
        keep, path_off, path, score, tok_off, start, end, logp, _gaps, stats = got
        for j, u in enumerate(keep):
            text, tok, wf, tlp, wlp = self._token_words(targets[u], start, end, logp, tok_off[j])
            out[u] = AlignedText(text, path[path_off[j]:path_off[j + 1]].copy(), float(score[j]), tok, wf, tlp, wlp)
        return out, stats

    def _alignment_call(self, what: str, logits_list: Any, targets: List[List[int]], fold: int, strict: bool, bp_budget: int,
                        segment_frames: Optional[int], tiles: Optional[Tuple[int, int, int]] = None, gaps: bool = False):
        """The native call of the five alignments -- ctcdec_align_batch (``segment_frames`` None), _long_batch, _tiled_batch
        (``tiles`` = (tile_groups, tile_frames, segment_blocks)) and, with ``gaps`` (-1 in a target), _gaps_batch and
        _gaps_long_batch -- on the utterances that have a path, and its results copied out. -> None when no call was made,
        else (keep; per kept utterance path_off and score, and the paths end to end; tok_off, and per label start, end and,
        with a fold, logp, else None; with ``gaps`` (gap_off, and per gap start, end, logp), else None; the stats: (timing ms,
        launches, plan) and, tiled, (counts, pass ms, tiled plan))."""
        if not targets:
            return None
        budget = bp_budget or ALIGN_BP_BUDGET
        if tiles is not None:
            entry, extra, table_name = "tiled_", tiles, "plan (column, edge rows, checkpoints; align_long without tiled needs less memory)"
            table_bytes = lambda T, L: self._align_tiled_plan(T, L, budget, *tiles)[5]  # noqa: E731
        elif segment_frames is None:
            entry, extra, table_name, table_bytes = "", (), "back-pointer table", self._bp_table_bytes
        else:
            entry, extra, table_name = "long_", (segment_frames,), "plan (segment table, checkpoints, columns)"
            table_bytes = lambda T, L: self._align_long_plan(T, L, budget, segment_frames)[2]  # noqa: E731
        with self._call_lock:
            batch, frames, ptrs, _ = self._stage_transcript_call(logits_list)
            keep, _k_frames, c_utts, flat, off = self._keep_feasible(what, frames, ptrs, targets, table_bytes, budget, strict,
                                                                   table_name, "path", gaps)
            if not keep:
                return None
            res = C.c_void_p()
            lib = self._lib
            lib.check(getattr(lib.dll, "ctcdec_align_%s%sbatch" % ("gaps_" if gaps else "", entry))(
                self._handle, *c_utts, len(keep), batch.dtype, int(batch.is_device), flat.ctypes.data_as(C.POINTER(C.c_int32)),
                B.off_ptr(off), fold, bp_budget, *extra, C.byref(res)))
            try:
                po, pp, ps, nu = B.read_out(lib, lib.dll.ctcdec_alignment_paths, res)
                to, _tl, ts, te, tp, nt = B.read_out(lib, lib.dll.ctcdec_alignment_tokens, res)
                n_lab = n_gap = ng = 0
                if gaps:
                    go, gs, ge, gl, ng = B.read_out(lib, lib.dll.ctcdec_alignment_gaps, res)
                    n_gap = int(np.count_nonzero(flat[:int(off[-1])] == -1))
                n_lab = int(off[-1]) - n_gap
                if nu != len(keep) or nt != n_lab or ng != n_gap:
                    raise B.NativeError("the alignment holds another number of utterances%s than was asked for"
                                        % (", tokens or gaps" if gaps else " or tokens"))
                path_off = B.values(po, len(keep) + 1)
                path, score = B.values(pp, path_off[-1], copy=True), B.values(ps, len(keep))
                tok_off = B.values(to, len(keep) + 1) if gaps else off.tolist()  # (without gaps every target entry is a token)
                start, end, logp = B.values(ts, n_lab), B.values(te, n_lab), B.values(tp, n_lab) if fold else None
                gap_values = (B.values(go, len(keep) + 1), B.values(gs, n_gap), B.values(ge, n_gap), B.values(gl, n_gap)) if gaps else None
                ms, launches = B.read_out(lib, lib.dll.ctcdec_alignment_timing, res, sizes=(4,))
                sf, ns, npl = B.read_out(lib, lib.dll.ctcdec_alignment_plan, res)
                stats = (ms, launches, list(zip(B.values(sf, npl), B.values(ns, npl))))
                if tiles is not None:
                    counts, ms2, p6, npl = B.read_out(lib, lib.dll.ctcdec_alignment_tiled, res, sizes=(4, 2))
                    stats += (counts, ms2, [tuple(row) for row in B.values(p6, (npl, 6))])
            finally:
                lib.dll.ctcdec_alignment_free(res)
        return keep, path_off, path, score, tok_off, start, end, logp, gap_values, stats

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

    @staticmethod
    def _align_tiled_plan(frames: int, n_labels: int, budget: int, tile_groups: int, tile_frames: int,
                          segment_blocks: int) -> Tuple[int, int, int, int, int, int, int, int]:
        """-> (GB, FB, nI, nJ, KB, bytes, K, n): how ctcdec_align_tiled_batch cuts an utterance (align_tiled_plan, csrc/ctc_align.h,
        the same rule): state blocks of GB groups of four states, time blocks of FB frames, segments of KB time blocks -- K =
        KB * FB frames, n of them --, and the bytes of the column, a ring of three time blocks per boundary between state blocks
        and a checkpoint for every segment but the first. The budget bounds the bytes and never changes the cut."""
        if frames <= 0:
            return 0, 0, 0, 0, 0, 0, 0, 0
        nch = (2 * n_labels + 1 + 3) // 4
        gb = tile_groups if tile_groups > 0 else SCORE_LONG_TILE_GROUPS
        n_i = -(-nch // gb)
        fb = min(tile_frames if tile_frames > 0 else SCORE_LONG_TILE_FRAMES, frames, ALIGN_TILED_MAX_SEGMENT)
        kb = segment_blocks if segment_blocks > 0 else ALIGN_TILED_MAX_SEGMENT // fb
        n = -(-frames // (kb * fb))
        return gb, fb, n_i, -(-frames // fb), kb, 8 * (4 * nch + 3 * (n_i - 1) * fb) + 32 * nch * (n - 1), kb * fb, n

    def align_long(self, logits: Any, text: Optional[str] = None, tokens: Optional[Sequence[int]] = None,
                   confidence: Optional[str] = None, tiled: bool = False) -> "AlignedText":
        """Forced alignment of one long utterance: align_long_batch of a batch of one (a ValueError when no path exists)."""
        _refuse_streams(logits, "align_long", "reads an utterance's matrix", batch=False)
        self._check_logits_dimension(logits)
        return self.align_long_batch([logits], None if text is None else [text], tokens=None if tokens is None else [tokens],
                                     confidence=confidence, tiled=tiled)[0]

    def align_long_batch(self, logits_list: Any, texts: Optional[Sequence[str]] = None,
                         tokens: Optional[Sequence[Sequence[int]]] = None, confidence: Optional[str] = None, strict: bool = True,
                         tiled: bool = False, _bp_budget: int = 0, _segment_frames: int = 0, _tile_groups: int = 0,
                         _tile_frames: int = 0, _segment_blocks: int = 0) -> List[Optional["AlignedText"]]:
        """align_batch for a lecture against its script: up to 1048575 target labels per utterance instead of 2047, and no
        back-pointer table of all frames (row_lse + ctc_viterbi_long, csrc/ctc_align_hip.hip). Arguments, targets, the
        probabilities-or-logits rule and ``strict`` are align_batch's, and for every input align_batch accepts the result is
        align_batch's, bit for bit. An utterance whose whole table fits the memory budget of a launch takes one pass; a longer
        one is cut into segments of about sqrt(32 T) frames and takes two: one that keeps the score column every segment
        starts from, one that fills and traces back one segment's table at a time, last segment first. The score columns
        live in device memory, so align_batch stays the faster call for targets it accepts. ``last_align_long_plan`` holds
        (segment_frames, n_segments) of every utterance aligned.

        ``tiled=True`` spreads one long utterance over many compute units (ctc_viterbi_tile + ctc_viterbi_cone): the states are
        cut into blocks of 256 groups of four and the frames into blocks of 64, a tile (state block, time block) runs on one
        workgroup and one launch takes a diagonal of tiles, as in score_long_batch; the column is kept every 448 frames, and a
        second pass restores, per segment and from the last to the first, only the states that can reach the path, and traces
        back. The result is the same, bit for bit. It takes more memory than the untiled plan (the checkpoints do not shrink)
        and is the slower call for a batch of many utterances, which fills the chip already. ``last_align_tiled_plan`` holds
        (tile_groups, tile_frames, state_blocks, time_blocks, segment_blocks, bytes) of every utterance aligned,
        ``last_align_tiled_launches`` and ``last_align_tiled_tiles`` the diagonals launched and the tiles in them."""
        _refuse_streams(logits_list, "align_long_batch", "reads utterances' matrices")
        fold = _confidence_fold(confidence)
        _bounded_int(_segment_frames, 0, 2 ** 31, "align_long: _segment_frames must be an int >= 0 (0: the library plans), not %r")
        if not isinstance(tiled, (bool, np.bool_)):
            raise ValueError("align_long: tiled must be a bool, not %r" % (tiled,))
        cut = (("_tile_groups", _tile_groups, SCORE_LONG_TILE_GROUPS + 1), ("_tile_frames", _tile_frames, 2 ** 31),
               ("_segment_blocks", _segment_blocks, 2 ** 31))
        for name, v, top in cut:
            _bounded_int(v, 0, top, "align_long: %s must be an int in [0, %d) (0: the library's rule), not %r", name, top)
            if v and not tiled:
                raise ValueError("align_long: %s cuts the tiles of tiled=True; without tiled there are none" % name)
        if tiled and _segment_frames:
            raise ValueError("align_long: _segment_frames cuts the untiled call; tiled=True takes _tile_frames and _segment_blocks")
        logits_list, targets = self._one_target_each("align_long", logits_list, texts, tokens, ALIGN_LONG_MAX_LABELS)
        out, stats = self._aligned_texts("align_long", logits_list, targets, fold, strict, int(_bp_budget), int(_segment_frames),
                                         tuple(int(v) for _name, v, _top in cut) if tiled else None)
        if stats is not None:
            self.last_align_long_timing_ms, self.last_align_long_launches, self.last_align_long_plan = stats[:3]
        if stats is not None and tiled:
            counts, self.last_align_tiled_pass_ms, self.last_align_tiled_plan = stats[3:]
            (self.last_align_tiled_launches, self.last_align_tiled_tiles, self.last_align_tiled_groups,
             self.last_align_tiled_widest) = counts
        return out

    # -- alignment with gaps (no reference analogue; DESIGN.md, "Alignment with gaps") --------------------
    def _gapped_targets(self, what: str, logits_list: Any, texts, tokens, gap: str, max_labels: int = ALIGN_MAX_LABELS):
        """-> (logits_list, items): the checks align_gaps_batch makes of its arguments before anything is staged -- one
        target per utterance, as a text (character alphabets) or as label ids, -1 standing for a gap; adjacent gaps merged."""
        if not isinstance(gap, str) or gap == "" or gap.split() != [gap]:
            raise ValueError("%s: the gap marker %r must be a non-empty string without whitespace" % (what, gap))
        if gap in self._vocab2idx:
            raise ValueError("%s: the gap marker %r is a label of the alphabet: choose another with gap=" % (what, gap))
        logits_list, given = self._targets_given(what, logits_list, texts, tokens)
        space = self._vocab2idx.get(" ")
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
                ids = self._label_ids(g, lambda _k: "%s: tokens[%d] holds" % (what, u), gap=True)
                if -1 in ids:  # (adjacent gaps are one)
                    ids = [c for k, c in enumerate(ids) if c != -1 or k == 0 or ids[k - 1] != -1]
            n_lab = len(ids) - ids.count(-1)
            if n_lab == 0:
                raise ValueError("%s: the target of utterance %d has no label: a gap alone aligns to everything" % (what, u))
            if n_lab > max_labels:
                raise ValueError("%s: utterance %d has %d target labels, above the limit of %d labels per utterance"
                                 % (what, u, n_lab, max_labels))
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
        out, stats = self._gapped_alignments("align_gaps", logits_list, targets, gap, fold, strict, int(_bp_budget), None)
        if stats is not None:
            # [classification (frame-prune kernels), row_lse_max, ctc_viterbi_gaps (HIP events), whole native call]
            self.last_align_gaps_timing_ms, self.last_align_gaps_launches, _plan = stats
        return out

    def _gapped_alignments(self, what: str, logits_list: Any, targets: List[List[int]], gap: str, fold: int, strict: bool,
                           bp_budget: int, segment_frames: Optional[int]):
        """-> (the GappedAlignment of every utterance, None for one without a path; the stats of the native call, None when
        none was made): the checked items through _alignment_call, and the words formed from the result."""
        out: List[Optional[GappedAlignment]] = [None] * len(targets)
        got = self._alignment_call(what, logits_list, targets, fold, strict, bp_budget, segment_frames, gaps=True)
        if got is None:
            return out, None
        keep, path_off, path, score, tok_off, start, end, logp, (gap_off, g_start, g_end, g_logp), stats = got
        for j, u in enumerate(keep):
            items, o = targets[u], tok_off[j]
            # the runs of labels between the gaps: each has its own words (a gap ends a word)
            parts, tok, wf, tlp, wlp, run = [], [], [], [], [], []
            for c in items + [-1]:
                if c != -1:
                    run.append(c)
                    continue
                if run:
                    text, run_tok, run_wf, run_tlp, run_wlp = self._token_words(run, start, end, logp, o)
                    tok += run_tok
                    wf += run_wf
                    if fold:
                        tlp += run_tlp
                        wlp += run_wlp
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
        return out, stats

    # -- alignment with gaps, long transcripts (no reference analogue; DESIGN.md, "Alignment with gaps, long transcripts") ----
    def align_gaps_long(self, logits: Any, text: Optional[str] = None, tokens: Optional[Sequence[int]] = None, gap: str = "*",
                        confidence: Optional[str] = None) -> "GappedAlignment":
        """Alignment of one long utterance to a transcript with gaps: align_gaps_long_batch of a batch of one."""
        _refuse_streams(logits, "align_gaps_long", "reads an utterance's matrix", batch=False)
        self._check_logits_dimension(logits)
        return self.align_gaps_long_batch([logits], None if text is None else [text], tokens=None if tokens is None else [tokens],
                                          gap=gap, confidence=confidence)[0]

    def align_gaps_long_batch(self, logits_list: Any, texts: Optional[Sequence[str]] = None,
                              tokens: Optional[Sequence[Sequence[int]]] = None, gap: str = "*", confidence: Optional[str] = None,
                              strict: bool = True, _bp_budget: int = 0, _segment_frames: int = 0) -> List[Optional["GappedAlignment"]]:
        """align_gaps_batch for a lecture against a script with holes: up to 1048575 target labels per utterance (gaps do not
        count) instead of 2047, and no back-pointer table of all frames (row_lse_max + ctc_viterbi_gaps_long,
        csrc/ctc_align_hip.hip). Targets, the gap marker, ``strict`` and the definition of a gap are align_gaps_batch's, and
        for every input align_gaps_batch accepts the result is that call's, bit for bit; a target without gaps gives
        align_long_batch's result. The frames are cut as align_long_batch cuts them, under the same budget;
        ``last_align_gaps_long_plan`` holds (segment_frames, n_segments) of every utterance aligned."""
        _refuse_streams(logits_list, "align_gaps_long_batch", "reads utterances' matrices")
        fold = _confidence_fold(confidence)
        _bounded_int(_segment_frames, 0, 2 ** 31, "align_gaps_long: _segment_frames must be an int >= 0 (0: the library plans), not %r")
        logits_list, targets = self._gapped_targets("align_gaps_long", logits_list, texts, tokens, gap, ALIGN_LONG_MAX_LABELS)
        out, stats = self._gapped_alignments("align_gaps_long", logits_list, targets, gap, fold, strict, int(_bp_budget),
                                             int(_segment_frames))
        if stats is not None:
            self.last_align_gaps_long_timing_ms, self.last_align_gaps_long_launches, self.last_align_gaps_long_plan = stats
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
                blob_p, off_p, nu = B.read_out(lib, lib.dll.ctcdec_greedy_texts, res)
                to, tl, ts, te, tp, ntok = B.read_out(lib, lib.dll.ctcdec_greedy_tokens, res)
                sp, ns = B.read_out(lib, lib.dll.ctcdec_greedy_scores, res)
                if nu != n or ns != n:
                    raise B.NativeError("the greedy result holds another number of utterances than was asked for")
                text_off = B.values(off_p, n + 1)
                blob = C.string_at(blob_p, text_off[n]) if text_off[n] else b""
                if blob.isascii():  # byte offsets == character offsets: decode once, slice the str
                    whole = blob.decode("ascii")
                    texts = [whole[text_off[k]:text_off[k + 1]] for k in range(n)]
                else:
                    texts = [blob[text_off[k]:text_off[k + 1]].decode("utf-8") for k in range(n)]
                offsets = B.values(to, n + 1, copy=True)
                if ntok != int(offsets[-1]):
                    raise B.NativeError("the greedy result holds another number of tokens than its offsets say")
                label, start, end = (B.values(q, ntok, copy=True) for q in (tl, ts, te))
                logp = score = None
                if fold:
                    logp, score = B.values(tp, ntok, copy=True), B.values(sp, n, copy=True)
                # [classification (frame-prune kernels), row_argmax / row_lse_argmax, greedy_collapse (HIP events), native call]
                self.last_greedy_timing_ms, self.last_greedy_launches, self.last_greedy_lse_ms = B.read_out(
                    lib, lib.dll.ctcdec_greedy_timing, res, sizes=(4,))
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
        ids = label.tolist()
        text, tok, wf, tlp, wlp = self._token_words(ids, start.tolist(), end.tolist(), logp.tolist() if fold else None)
        if text != texts[0]:
            raise B.NativeError("the native text %r differs from the text of the greedy labels %r" % (texts[0], text))
        return GreedyText(text, ids, tok, wf, tlp, wlp, float(score[0]) if fold else None)

    def _many_targets_each(self, what: str, item: str, items: str, logits_list: Any, texts, tokens, ids_of_text=None,
                           max_labels: int = ALIGN_MAX_LABELS):
        """The label ids of any number of given texts or token lists per utterance, checked: (logits_list, ids[u][j]).
        ``ids_of_text``: how a text becomes label ids (_target_of_text unless given)."""
        ids_of_text = ids_of_text or self._target_of_text
        logits_list, given = self._targets_given(what, logits_list, texts, tokens, items)
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
                    # (_label_ids' own short cut -- keep the two conditions the same --, taken here without the call: a batch
                    # holds tens of thousands of items, and a Python call for each is a measurable part of prefix_scores_batch)
                    if not (set(map(type, ids)) <= {int} and (not ids or (0 <= min(ids) and max(ids) < n_labels and blank not in ids))):
                        ids = self._label_ids(ids, lambda _k: "%s: %s holds" % (what, who))
                if len(ids) > max_labels:
                    raise ValueError("%s: %s has %d labels, above the limit of %d labels per %s"
                                     % (what, who, len(ids), max_labels, item))
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
        out, stats = self._scored_texts("score", logits_list, texts, tokens, with_lm, None)
        # [classification (frame-prune kernels), row_lse, forward kernels (HIP events), whole native call]; hypotheses that
        # went to (ctc_forward_wave, ctc_forward)
        self.last_score_timing_ms, self.last_score_launched = stats
        return out

    def _scored_texts(self, what: str, logits_list: Any, texts, tokens, with_lm: bool, tiles: Optional[Tuple[int, int, int]]):
        """-> (the ScoredText of every hypothesis of every utterance; what the native call did): the checked hypotheses
        through ctcdec_score_batch (``tiles`` None: (timing ms, hypotheses by kernel)) or ctcdec_score_long_batch (``tiles``
        its budget, tile_groups and tile_frames: (timing ms, (diagonals, tiles, launch groups, widest diagonal), plans)), and the language
        model's term."""
        lm = self._language_model
        if with_lm and lm is None:
            raise ValueError("%s: with_lm=True needs a decoder with a language model" % what)
        logits_list, hyps = self._many_targets_each(what, "hypothesis", "hypotheses", logits_list, texts, tokens,
                                                    max_labels=ALIGN_MAX_LABELS if tiles is None else ALIGN_LONG_MAX_LABELS)
        zeros = (0.0, 0.0, 0.0, 0.0)
        n = len(hyps)
        if n == 0:
            return [], ((zeros, (0, 0)) if tiles is None else (zeros, (0, 0, 0, 0), []))
        kernel = _forced_kernel("CTCDEC_FORWARD_KERNEL", FORWARD_KERNELS)
        with self._call_lock:
            batch, frames, ptrs, c_utts = self._stage_transcript_call(logits_list)
            if tiles is not None:
                budget = tiles[0] or ALIGN_BP_BUDGET
                for u, cur in enumerate(hyps):
                    for k, ids in enumerate(cur):
                        need = self._score_long_plan(int(frames[u]), len(ids), budget, tiles[1], tiles[2])[4]
                        if need > budget and int(frames[u]) >= self._frames_needed(ids):
                            raise ValueError("%s: utterance %d, hypothesis %d needs a column and edge rows of %d bytes, above the "
                                             "memory budget of %d bytes of one launch" % (what, u, k, need, budget))
            flat, target_off, hyp_off, nh = self._pack_items(hyps)
            logp = np.zeros(max(nh, 1), dtype=np.float64)
            ms = (C.c_double * 4)()
            lib = self._lib
            head = (self._handle, *c_utts, n, batch.dtype, int(batch.is_device), flat.ctypes.data_as(C.POINTER(C.c_int32)),
                    B.off_ptr(target_off), B.off_ptr(hyp_off))
            if tiles is None:
                launched = (C.c_int64 * 2)()
                lib.check(lib.dll.ctcdec_score_batch(*head, kernel, logp.ctypes.data_as(C.POINTER(C.c_double)), ms, launched))
                stats = (tuple(float(v) for v in ms), (int(launched[0]), int(launched[1])))
            else:
                counts, plan = (C.c_int64 * 5)(), np.zeros((max(nh, 1), 5), dtype=np.int64)
                lib.check(lib.dll.ctcdec_score_long_batch(*head, *tiles, logp.ctypes.data_as(C.POINTER(C.c_double)), ms, counts,
                                                          plan.ctypes.data_as(C.POINTER(C.c_int64))))
                stats = (tuple(float(v) for v in ms), (int(counts[0]), int(counts[1]), int(counts[2]), int(counts[4])),
                         [tuple(row) for row in plan[:int(counts[3])].tolist()])
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
        return out, stats

    # -- transcript likelihood of long transcripts (no reference analogue; DESIGN.md, "Transcript likelihood of long transcripts")
    @staticmethod
    def _score_long_plan(frames: int, n_labels: int, budget: int, tile_groups: int, tile_frames: int) -> Tuple[int, int, int, int, int]:
        """-> (tile_groups, tile_frames, state_blocks, time_blocks, bytes): how ctcdec_score_long_batch cuts a hypothesis
        (score_long_plan, csrc/ctc_align.h, the same rule): state blocks of GB groups of four states, time blocks of FB frames,
        and the bytes of its column and of a ring of three time blocks per boundary between state blocks."""
        if frames <= 0:
            return 0, 0, 0, 0, 0
        nch = (2 * n_labels + 1 + 3) // 4
        gb = tile_groups if tile_groups > 0 else SCORE_LONG_TILE_GROUPS
        n_i = -(-nch // gb)
        rows = 3 * (n_i - 1)
        fb = tile_frames if tile_frames > 0 else frames if n_i == 1 else SCORE_LONG_TILE_FRAMES
        if tile_frames <= 0 and rows > 0 and 8 * (4 * nch + rows * fb) > budget:
            fb = (budget // 8 - 4 * nch) // rows
        fb = max(1, min(fb, frames))
        return gb, fb, n_i, -(-frames // fb), 8 * (4 * nch + rows * fb)

    def score_long(self, logits: Any, texts: Optional[Sequence[str]] = None, tokens: Optional[Sequence[Sequence[int]]] = None,
                   with_lm: bool = False) -> List["ScoredText"]:
        """The likelihood of each long hypothesis for one utterance: score_long_batch of a batch of one."""
        _refuse_streams(logits, "score_long", "reads an utterance's matrix", batch=False)
        self._check_logits_dimension(logits)
        return self.score_long_batch([logits], None if texts is None else [texts], tokens=None if tokens is None else [tokens],
                                     with_lm=with_lm)[0]

    def score_long_batch(self, logits_list: Any, texts: Optional[Sequence[Sequence[str]]] = None,
                         tokens: Optional[Sequence[Sequence[Sequence[int]]]] = None, with_lm: bool = False, _budget: int = 0,
                         _tile_groups: int = 0, _tile_frames: int = 0) -> List[List["ScoredText"]]:
        """score_batch for a lecture against its script: up to 1048575 labels per hypothesis instead of 2047 (row_lse +
        ctc_forward_tile, csrc/ctc_align_hip.hip). Arguments, hypotheses, the -inf rule and ``with_lm`` are score_batch's, and
        for every input score_batch accepts ``logp`` is score_batch's, bit for bit. A hypothesis' states are cut into blocks
        of 256 groups of four and its frames into blocks of 64; a tile (state block, time block) runs on one workgroup, and
        one launch takes a diagonal of tiles, so a long hypothesis spreads over many compute units. score_batch stays the
        faster call for hypotheses it accepts. ``last_score_long_plan`` holds (tile_groups, tile_frames, state_blocks,
        time_blocks, bytes) of every hypothesis launched, ``last_score_long_launches`` and ``last_score_long_tiles`` the
        diagonals launched and the tiles in them, ``last_score_long_groups`` the launch groups the budget made, ``last_score_long_widest`` the most tiles one diagonal held."""
        _refuse_streams(logits_list, "score_long_batch", "reads utterances' matrices")
        for name, v, top in (("_budget", _budget, 2 ** 63), ("_tile_groups", _tile_groups, SCORE_LONG_TILE_GROUPS + 1),
                             ("_tile_frames", _tile_frames, 2 ** 31)):
            _bounded_int(v, 0, top, "score_long: %s must be an int in [0, %d) (0: the library's rule), not %r", name, top)
        out, stats = self._scored_texts("score_long", logits_list, texts, tokens, with_lm,
                                        (int(_budget), int(_tile_groups), int(_tile_frames)))
        self.last_score_long_timing_ms, counts, self.last_score_long_plan = stats
        self.last_score_long_launches, self.last_score_long_tiles, self.last_score_long_groups, self.last_score_long_widest = counts
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
        self._set_call_stats("prefix", (0.0,) * 5, (0, 0, 0), (0, 0))
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
                end_p, next_p, n_prefixes, n_next = B.read_out(lib, lib.dll.ctcdec_prefix_scores, res)
                if n_prefixes != nh or n_next != n_labels:
                    raise B.NativeError("the prefix result holds another number of scores than was asked for")
                ends = B.values(end_p, nh)
                if buf is None:
                    buf = B.values(next_p, (nh, n_labels), copy=True)
                # [classification (frame-prune kernels), row_lse, forward kernels with end states, ctc_prefix_extend (HIP
                # events), whole native call]; prefixes that went to (ctc_forward_wave_ends, ctc_forward_ends)
                self._set_call_stats("prefix", *B.read_out(lib, lib.dll.ctcdec_prefix_timing, res, sizes=(5, 3, 2)))
            finally:
                lib.dll.ctcdec_prefix_free(res)
            if batch.is_device:
                self.last_prefix_next = buf
        space = None if self._is_bpe else self._vocab2idx.get(" ")
        rows = buf.unbind(0) if batch.is_device else list(buf)  # (every row's view in one call)
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
        _refuse_streams(logits, "find", "searches an utterance's matrix", batch=False)
        self._check_logits_dimension(logits)
        return self.find_batch([logits], None if texts is None else [texts], tokens=None if tokens is None else [tokens],
                               max_hits=max_hits, min_logp=min_logp, trace=trace)[0]

    def _set_call_stats(self, name: str, timing_ms, launches, launched) -> None:
        """The diagnostics of the last call of a kind, where they are these three (_init_transcript_stats says what each holds)"""
        setattr(self, "last_%s_timing_ms" % name, timing_ms)
        setattr(self, "last_%s_launches" % name, launches)
        setattr(self, "last_%s_launched" % name, launched)

    def _search_batch(self, name: str, result, hit, logits_list: Any, texts, tokens, max_hits, min_logp, trace, _trace_budget):
        """find_batch ("find": ctcdec_find_batch, PhraseSearch of PhraseHit) and spot_batch ("spot": ctcdec_spot_batch,
        PhraseSpot of SpotHit, with the phrases' counts): the checks, the native call and the results formed from it."""
        _refuse_streams(logits_list, "%s_batch" % name, "searches utterances' matrices")
        logits_list, phrases = self._many_targets_each(name, "phrase", "phrases", logits_list, texts, tokens)
        for u, cur in enumerate(phrases):
            for j, ids in enumerate(cur):
                if not ids:
                    raise ValueError("%s: utterance %d, phrase %d is empty: it would occur everywhere and nowhere" % (name, u, j))
        max_hits = _bounded_int(max_hits, 1, FIND_MAX_HITS + 1, "%s: max_hits must be an int in 1 .. %d, not %r", name, FIND_MAX_HITS)
        floor = -math.inf if min_logp is None else float(min_logp)
        if math.isnan(floor):
            raise ValueError("%s: min_logp is not a number" % name)
        n = len(phrases)
        self._set_call_stats(name, (0.0, 0.0, 0.0, 0.0), 0, (0, 0))
        if n == 0:
            return []
        kernel = _forced_kernel("CTCDEC_FIND_KERNEL", FIND_KERNELS)
        with self._call_lock:
            batch, frames, ptrs, c_utts = self._stage_transcript_call(logits_list)
            budget = int(_trace_budget) or ALIGN_BP_BUDGET
            for u, cur in enumerate(phrases):
                for j, ids in enumerate(cur):
                    if int(frames[u]) >= self._frames_needed(ids) and 12 * int(frames[u]) > budget:
                        raise ValueError("%s: utterance %d, phrase %d needs a trace of %d bytes, above the memory budget of %d "
                                         "bytes of one launch" % (name, u, j, 12 * int(frames[u]), budget))
            flat, label_off, hyp_off, n_phrases = self._pack_items(phrases)
            res = C.c_void_p()
            lib = self._lib
            lib.check(getattr(lib.dll, "ctcdec_%s_batch" % name)(
                self._handle, *c_utts, n,
                batch.dtype, int(batch.is_device), B.off_ptr(hyp_off), B.off_ptr(label_off), flat.ctypes.data_as(C.POINTER(C.c_int32)),
                max_hits, floor, int(bool(trace)), kernel, int(_trace_budget), C.byref(res)))
            try:
                ho, ps, pe, pl, nph = B.read_out(lib, lib.dll.ctcdec_search_hits, res)
                if nph != n_phrases:
                    raise B.NativeError("the search holds another number of phrases than was asked for")
                hit_off = B.values(ho, n_phrases + 1)
                starts, ends, logps = B.values(ps, hit_off[-1]), B.values(pe, hit_off[-1]), B.values(pl, hit_off[-1])
                if trace:
                    to, tl, ts = B.read_out(lib, lib.dll.ctcdec_search_trace, res)
                    t_off = B.values(to, n_phrases + 1)
                    t_logp, t_start = B.values(tl, t_off[-1], copy=True), B.values(ts, t_off[-1], copy=True)
                counts = None
                if name == "spot":
                    counts = B.values(B.read_out(lib, lib.dll.ctcdec_search_count, res)[0], n_phrases)
                # [classification (frame-prune kernels), row_lse, the call's kernels (HIP events), whole native call]; kernel
                # launches made; phrases that went to (the wave kernel, the group kernel)
                self._set_call_stats(name, *B.read_out(lib, lib.dll.ctcdec_search_timing, res, sizes=(4, 0, 2)))
            finally:
                lib.dll.ctcdec_search_free(res)
        out, h = [], 0
        for cur in phrases:
            found = []
            for ids in cur:
                hits = [hit(starts[k], ends[k], logps[k]) for k in range(hit_off[h], hit_off[h + 1])]
                el = es = None
                if trace:
                    el, es = t_logp[t_off[h]:t_off[h + 1]].copy(), t_start[t_off[h]:t_off[h + 1]].copy()
                count = () if counts is None else (counts[h],)  # (PhraseSpot's extra field)
                found.append(result(self._words_of_target(ids)[0], list(ids), hits, *count, el, es))
                h += 1
            out.append(found)
        return out

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
        return self._search_batch("find", PhraseSearch, PhraseHit, logits_list, texts, tokens, max_hits, min_logp, trace, _trace_budget)

    # -- phrase spotting (no reference analogue; DESIGN.md, "Phrase spotting") ------------------------------
    def spot(self, logits: Any, texts: Optional[Sequence[str]] = None, tokens: Optional[Sequence[Sequence[int]]] = None,
             max_hits: int = 1, min_logp: Optional[float] = None, trace: bool = False) -> List["PhraseSpot"]:
        """The probability that each phrase occurs in one utterance, and where: spot_batch of a batch of one."""
        _refuse_streams(logits, "spot", "searches an utterance's matrix", batch=False)
        self._check_logits_dimension(logits)
        return self.spot_batch([logits], None if texts is None else [texts], tokens=None if tokens is None else [tokens],
                               max_hits=max_hits, min_logp=min_logp, trace=trace)[0]

    def spot_batch(self, logits_list: Any, texts: Optional[Sequence[Sequence[str]]] = None,
                   tokens: Optional[Sequence[Sequence[Sequence[int]]]] = None, max_hits: int = 1,
                   min_logp: Optional[float] = None, trace: bool = False, _trace_budget: int = 0) -> List[List["PhraseSpot"]]:
        """How probable is it that each phrase occurs in its utterance, summed over every alignment, in one native call:
        find_batch's arguments, per phrase a PhraseSpot (row_lse once per utterance + ctc_spot / ctc_spot_wave,
        csrc/ctc_align_hip.hip). Per end frame ``t`` the call forms the log-probability that an occurrence of the phrase --
        a window that begins on a frame of the first label not preceded by that label, collapses to exactly the phrase, and
        ends on a frame of the last label not followed by that label -- ends on ``t``, and the mass-weighted mean start frame
        of those occurrences; ``count`` is the sum of the probabilities over the end frames, the expected number of
        occurrences. The hits are find_batch's selection on that trace: up to ``max_hits`` (1 .. 64) pairwise disjoint
        windows ``[mean start, t]``, most probable end frame first, none below ``min_logp``. ``trace=True`` also returns
        the per-frame ``end_logp`` / ``end_start``. ``CTCDEC_FIND_KERNEL=wave|group`` applies as it does to find_batch."""
        return self._search_batch("spot", PhraseSpot, SpotHit, logits_list, texts, tokens, max_hits, min_logp, trace, _trace_budget)

    def spot_streams(self, texts: Optional[Sequence[Any]] = None, tokens: Optional[Sequence[Any]] = None,
                     n_streams: Optional[int] = None, max_frames: Optional[int] = None) -> "SpotStreams":
        """spot_batch for live audio: a SpotStreams session whose ``feed`` takes one chunk per stream and returns the entries
        of spot_batch's trace that became final, the states of every phrase kept on the device in between (kernel
        ctc_spot_chunk, csrc/ctc_align_hip.hip; DESIGN.md, "Phrase spotting on streams"). ``texts`` / ``tokens``: one list of
        phrases per stream, or, with ``n_streams``, one flat list that every stream shares; 1 .. 127 labels per phrase.
        ``max_frames`` keeps a device trace of that many frames per phrase for ``hits()``; a stream cannot be fed past it.
        ``CTCDEC_SPOT_STREAM_WIDTH=64`` gives every phrase a wavefront of its own instead of packing short ones."""
        return SpotStreams(self, texts, tokens, n_streams, max_frames)

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
        self._set_call_stats("posteriors", (0.0,) * 4, 0, (0, 0))
        if n == 0:
            return []
        with self._call_lock:
            batch, frames, ptrs, _ = self._stage_transcript_call(logits_list)
            keep, _k_frames, c_utts, flat, off = self._keep_feasible("posteriors", frames, ptrs, targets, self._state_table_bytes,
                                                                   int(_table_budget) or POSTERIORS_TABLE_BUDGET, strict)
            out: List[Optional[TranscriptPosteriors]] = [None] * n
            if not keep:
                return out
            res = C.c_void_p()
            lib = self._lib
            lib.check(lib.dll.ctcdec_posteriors_batch(
                self._handle, *c_utts,
                len(keep), batch.dtype, int(batch.is_device), B.off_ptr(off), flat.ctypes.data_as(C.POINTER(C.c_int32)),
                int(bool(dense)), int(_table_budget), C.byref(res)))
            try:
                pl, pb, nu = B.read_out(lib, lib.dll.ctcdec_posteriors_scores, res)
                _to, po, pc, ntok = B.read_out(lib, lib.dll.ctcdec_posteriors_tokens, res)
                go, gs, gp = B.read_out(lib, lib.dll.ctcdec_posteriors_gamma, res)
                if nu != len(keep) or ntok != int(off[-1]):
                    raise B.NativeError("the posteriors hold another number of utterances or tokens than was asked for")
                logp, logp_b = B.values(pl, len(keep)), B.values(pb, len(keep))
                occ, cen = B.values(po, ntok, copy=True), B.values(pc, ntok, copy=True)
                gammas: List[Optional[np.ndarray]] = [None] * len(keep)
                if dense:
                    g_off, stride = B.values(go, len(keep) + 1), B.values(gs, len(keep))
                    # (a view of the library's rows, not a second copy of them: each utterance's part is copied out below)
                    flat_g = np.ctypeslib.as_array(gp, shape=(g_off[-1],)) if g_off[-1] else np.zeros(0)
                    for j, u in enumerate(keep):
                        T, S = int(frames[u]), 2 * len(targets[u]) + 1
                        gammas[j] = flat_g[g_off[j]:g_off[j + 1]].reshape(T, stride[j])[:, :S].copy()
                # [classification (frame-prune kernels), row_lse, ctc_posteriors (HIP events), whole native call]; kernel
                # launches made; utterances that went to (the 256-thread kernel, the 1024-thread kernel)
                self._set_call_stats("posteriors", *B.read_out(lib, lib.dll.ctcdec_posteriors_timing, res, sizes=(4, 0, 2)))
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
        self._set_call_stats("gradient", (0.0,) * 5, 0, (0, 0))
        if n == 0:
            return [], None, []
        with self._call_lock:
            batch, frames, ptrs, _ = self._stage_transcript_call(logits_list)
            keep, k_frames, c_utts, flat, off = self._keep_feasible("gradient", frames, ptrs, targets, self._state_table_bytes,
                                                                  int(_table_budget) or POSTERIORS_TABLE_BUDGET, strict)
            out: List[Optional[TranscriptGradient]] = [None] * n
            if not keep:
                return out, None, keep
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
                self._handle, *c_utts,
                len(keep), batch.dtype, int(batch.is_device), B.off_ptr(off), flat.ctypes.data_as(C.POINTER(C.c_int32)),
                g_ptrs.ctypes.data_as(C.POINTER(C.c_void_p)), 1 if wide else 0, int(_table_budget),
                logp.ctypes.data_as(C.POINTER(C.c_double)), ms, C.byref(launches), launched))
            # [classification (frame-prune kernels), row_lse, ctc_posteriors, ctc_grad_rows (HIP events), whole native call];
            # kernel launches made (both kernels); utterances that went to (the 256-thread, the 1024-thread) ctc_posteriors
            self._set_call_stats("gradient", tuple(ms), launches.value, tuple(launched))
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
