"""MI355X-native CTC beam-search decoder with the pyctcdecode API surface
(reference exports: pyctcdecode/__init__.py:2-4)."""
from .alphabet import Alphabet  # noqa: F401
from .decoder import (ALIGN_LONG_MAX_LABELS, AlignedText, BeamSearchDecoderCTC, ConfidenceLMBeam, ConfidenceOutputBeam, GappedAlignment, GreedyFrames,  # noqa: F401
                      GreedyText, PhraseHit, PhraseSearch, PrefixScores, PrefixSession, ScoredText, SessionPrefix, TokenFrames, TokenLMBeam,
                      TokenOutputBeam, TranscriptGradient, TranscriptPosteriors, build_ctcdecoder)
from .language_model import LanguageModel  # noqa: F401

__version__ = "0.1.0"
