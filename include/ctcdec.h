/*
 * ctcdec.h -- C ABI of libctcdec.so, the MI355X-native CTC prefix-beam-search decoder.
 *
 * The reference (kensho-technologies/pyctcdecode) is pure Python and has NO FFI: its boundary for
 * this path is the Python surface BeamSearchDecoderCTC.decode / decode_beams / decode_batch /
 * decode_beams_batch (pyctcdecode/decoder.py:730-945) built by build_ctcdecoder
 * (decoder.py:1051-1099).  This header is the C ABI a maintainer would bind underneath that
 * surface (ctypes stub: INTEGRATION.md); every entry point cites the reference code it replaces.
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on success and a
 * negative ctcdec_status otherwise (never throws); ctcdec_last_error() returns a thread-local
 * message.  The caller owns all input buffers; the library owns result objects until
 * ctcdec_result_free().  One decoder handle may be used from one host thread at a time.
 */
#ifndef CTCDEC_H
#define CTCDEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ctcdec_decoder ctcdec_decoder; /* opaque */
typedef struct ctcdec_result ctcdec_result;   /* opaque */

enum ctcdec_status {
  CTCDEC_OK = 0,
  CTCDEC_ERR_ARG = -1,     /* bad argument (ValueError on the Python side)            */
  CTCDEC_ERR_IO = -2,      /* cannot read / parse the LM file                          */
  CTCDEC_ERR_DEVICE = -3,  /* HIP runtime failure or no gfx950 device                  */
  CTCDEC_ERR_LIMIT = -4,   /* request exceeds a documented limit (beam width, order..) */
  CTCDEC_ERR_INTERNAL = -5
};

enum ctcdec_dtype { CTCDEC_F32 = 0, CTCDEC_F64 = 1, CTCDEC_F16 = 2, CTCDEC_BF16 = 3 };  /* host or device pointers alike (host float16 matrices are staged as they are) */

/* Maximum supported values (checked; CTCDEC_ERR_LIMIT otherwise). */
#define CTCDEC_MAX_BEAM_WIDTH 256
#define CTCDEC_MAX_LM_ORDER 6
#define CTCDEC_MAX_VOCAB 65535
#define CTCDEC_MAX_LMS 4 /* language models in one MultiLanguageModel */

/* Decode-time parameters: the keyword arguments of decode_beams (decoder.py:730-740) plus the
 * LM parameters that reset_params may change between calls (decoder.py:292-313,
 * language_model.py:271-301), which is why they are per-call kernel arguments. */
typedef struct ctcdec_params {
  int32_t beam_width;        /* DEFAULT_BEAM_WIDTH 100       constants.py:8  */
  int32_t prune_history;     /* 0/1; decode() forces 1       decoder.py:888  */
  int32_t n_best;            /* beams to return per utterance (<=0: all, 1 for decode()) */
  int32_t want_lm_state;     /* 0/1: also return last_lm_state per beam      */
  double beam_prune_logp;    /* DEFAULT_PRUNE_LOGP -10       constants.py:10 */
  double token_min_logp;     /* DEFAULT_MIN_TOKEN_LOGP -5    constants.py:12 */
  double hotword_weight;     /* DEFAULT_HOTWORD_WEIGHT 10    constants.py:9  */
  double alpha;              /* language_model.py:266        */
  double beta;               /* language_model.py:267        */
  double unk_score_offset;   /* language_model.py:268        */
  double log_base_change;    /* LOG_BASE_CHANGE_FACTOR       constants.py:18 */
  int32_t lm_score_boundary; /* language_model.py:269        */
  int32_t first_frame;       /* processed_frames offset      decoder.py:443  */
  int32_t texts_only;        /* 0/1 (ctcdec_decode_batch with n_best = 1): only the best beam's TEXT is wanted
                                (decode_batch, decoder.py:895-945) -- it is assembled on the device and the result holds
                                one beam per utterance with its text and scores, no word frames and no LM state */
  int32_t token_frames;      /* 0/1: also keep every returned beam's tokens with their frames for
                                ctcdec_result_token_frames (takes precedence over texts_only); was a reserved 0.
                                CTCDEC_TOKEN_LOGP_MEAN / _MIN / _MAX: the same, plus each token's confidence for
                                ctcdec_result_token_logp (ctcdec_decode_batch, and ctcdec_stream_push / _read of streams
                                whose first chunk asked for the fold; not ctcdec_decode_stream_batch) */
} ctcdec_params;

/* ctcdec_params.token_frames beyond 0/1: the fold of a token's per-frame log-probabilities (ctcdec_result_token_logp) */
enum ctcdec_token_logp { CTCDEC_TOKEN_LOGP_MEAN = 2, CTCDEC_TOKEN_LOGP_MIN = 3, CTCDEC_TOKEN_LOGP_MAX = 4 };

/* LM start state for one utterance (decode_beams(lm_start_state=...), decoder.py:621-625):
 * context words newest first, as vocabulary indices of THIS decoder's LM, with the back-off
 * weight of each context length. length == -1 means "use the LM's own start state". */
typedef struct ctcdec_lm_state {
  int32_t length;
  uint32_t words[CTCDEC_MAX_LM_ORDER - 1];
  float backoff[CTCDEC_MAX_LM_ORDER - 1];
} ctcdec_lm_state;

/* ---- construction: replaces BeamSearchDecoderCTC.__init__ / build_ctcdecoder ------------------
 * labels_blob/labels_off: the NORMALISED alphabet (Alphabet.labels, alphabet.py:139-148) as one
 * UTF-8 blob with n_labels+1 byte offsets; is_bpe = Alphabet.is_bpe.  device: HIP device index. */
int ctcdec_create(const char* labels_blob, const int64_t* labels_off, int32_t n_labels,
                  int32_t is_bpe, int32_t device, ctcdec_decoder** out);
void ctcdec_destroy(ctcdec_decoder* dec);

/* Replaces kenlm.Model(path) (decoder.py:1074): parse an ARPA file into the flat hashed n-gram
 * trie and upload it.  order_out receives the n-gram order (LanguageModel.order). */
int ctcdec_lm_load_arpa(ctcdec_decoder* dec, const char* path, int32_t* order_out);

/* The parsed model as one flat file (vocabulary, unigram array and the hashed n-gram table in upload
 * layout): what a kenlm binary is to an ARPA file (language_model.py:424 accepts .bin/.binary next to
 * .arpa) -- loading is a few reads instead of a parse.  (kenlm's own probing binaries: ctcdec_lm_load_kenlm below.) */
int ctcdec_lm_save_flat(const ctcdec_decoder* dec, const char* path);
int ctcdec_lm_load_flat(ctcdec_decoder* dec, const char* path, int32_t* order_out);

/* Replaces kenlm.Model("x.bin") (decoder.py:1074; language_model.py:424 accepts .bin / .binary): a kenlm PROBING binary
 * (`build_binary probing`) -- header and sanity block, vocabulary strings checked against the vocabulary hash table, the
 * unigram array and the per-order probing tables adopted entry by entry into the flat trie (which uses kenlm's own n-gram key
 * chain for that reason).  Trie / quantised / array-compressed / rest-cost models are refused by name (CTCDEC_ERR_IO).
 * FORMAT UNPINNED AGAINST REAL KENLM: restated from the published sources, pinned against ctcdec_arpa_to_kenlm_binary only
 * (csrc/kenlm_binary.cpp).  ctcdec_is_kenlm_binary: 1 when the file starts with kenlm's magic bytes. */
int ctcdec_lm_load_kenlm(ctcdec_decoder* dec, const char* path, int32_t* order_out);
int ctcdec_is_kenlm_binary(const char* path);
/* ARPA -> kenlm probing binary (what `build_binary probing x.arpa x.bin` writes, as far as kenlm's sources say): a converter
 * and the reader's test vector.  probing_multiplier <= 1: kenlm's default 1.5. */
int ctcdec_arpa_to_kenlm_binary(const char* arpa_path, const char* out_path, float probing_multiplier);

/* Replaces LanguageModel.__init__'s unigram handling (language_model.py:257-265, :87-103):
 * unigrams given as a UTF-8 blob + offsets; has_unigrams=0 means "unigrams is None" (no trie).
 * Words not in the LM vocabulary are dropped (language_model.py:95).  n_kept_out: |unigram_set|. */
int ctcdec_lm_set_unigrams(ctcdec_decoder* dec, int32_t has_unigrams, const char* blob,
                           const int64_t* off, int64_t n_unigrams, int64_t* n_kept_out);

/* Let `dst` use the language model already loaded into `src` (shared, reference counted): a
 * LanguageModel object constructed on its own (language_model.py:237-269) and later handed to
 * BeamSearchDecoderCTC(alphabet, language_model) (decoder.py:275-290) is parsed only once. */
int ctcdec_lm_share(ctcdec_decoder* dst, const ctcdec_decoder* src);

/* Give `dst` a private COPY of the language model loaded into `src`. The reference builds many LanguageModels with
 * different unigram sets on one immutable kenlm.Model (tests/test_decoder.py:188-280); here the unigram set lives
 * in the model's prefix table, so every LanguageModel after the first gets its own copy instead of rewriting the
 * tables under the decoders that share the first one. */
int ctcdec_lm_clone(ctcdec_decoder* dst, const ctcdec_decoder* src);

/* Replaces MultiLanguageModel (language_model.py:455-502): `dst` scores every word with the n
 * (2..CTCDEC_MAX_LMS) language models loaded into srcs[0..n) -- each from its own state, the scores
 * averaged (language_model.py:483-502), partial words by the mean of the models' unigram-trie scores
 * (:477-481), history pruning by the largest order (:467-469). Model 0 takes alpha / beta /
 * unk_score_offset / lm_score_boundary from ctcdec_params like a single model; models 1.. take theirs
 * from ctcdec_lm_set_params (each reference LanguageModel carries its own, language_model.py:266-269).
 * With several models every "LM state" of the decode calls is n consecutive ctcdec_lm_state entries
 * in model order: start_states holds n per utterance, ctcdec_result_lm_state_of reads model k's; a streaming
 * beam (ctcdec_decode_stream_batch) carries the states of models 1.. in ctcdec_beam_in.more_states. */
int ctcdec_lm_share_multi(ctcdec_decoder* dst, const ctcdec_decoder* const* srcs, int32_t n);
int ctcdec_lm_set_params(ctcdec_decoder* dec, int32_t k /* 1..n-1 */, double alpha, double beta,
                         double unk_score_offset, int32_t lm_score_boundary);
/* number of language models behind the decoder (0: none) */
int ctcdec_lm_count(const ctcdec_decoder* dec, int32_t* n_out);

/* Unigram char-trie query: CharTrie.has_node (language_model.py:331) and set membership
 * (language_model.py:351).  flags_out: bit0 prefix of a unigram, bit1 LM vocabulary word,
 * bit2 member of the unigram set. */
int ctcdec_lm_prefix_flags(const ctcdec_decoder* dec, const char* str_utf8, int64_t len,
                           uint32_t* flags_out);

/* kenlm vocabulary queries used by the Python shell: Model.__contains__ (language_model.py:95,
 * 352) and word index / word string for exporting and importing LM states. */
int ctcdec_lm_word_index(const ctcdec_decoder* dec, const char* word_utf8, int64_t len,
                         uint32_t* index_out);
int ctcdec_lm_word_string(const ctcdec_decoder* dec, uint32_t index, const char** str_out,
                          int64_t* len_out);

/* Host-side single-word query = kenlm.Model.BaseScore (language_model.py:347) and the start
 * states BeginSentenceWrite / NullContextWrite (language_model.py:311-314).  Used by the public
 * LanguageModel.score()/get_start_state() methods, NOT by the decode path (which runs on device). */
int ctcdec_lm_start_state(const ctcdec_decoder* dec, int32_t begin_sentence, ctcdec_lm_state* out);
int ctcdec_lm_base_score(const ctcdec_decoder* dec, const ctcdec_lm_state* in, uint32_t word_index,
                         ctcdec_lm_state* out, float* log10_prob_out);

/* Replaces HotwordScorer.build_scorer (language_model.py:152-189) for the next decode calls:
 * hot-word UNIGRAMS (already stripped and split by the caller) as UTF-8 blob + offsets. */
int ctcdec_set_hotwords(ctcdec_decoder* dec, const char* blob, const int64_t* off, int64_t n_words);

/* Per-utterance hot words for the NEXT decode call on this handle only (ctcdec_decode_batch, ctcdec_decode_stream_batch,
 * ctcdec_stream_push, ctcdec_stream_import); that call takes them whatever its outcome, and the call after it is back on
 * the set of ctcdec_set_hotwords, which keeps its meaning.  Set k = unigrams [set_off[k], set_off[k+1]) of blob / off
 * (already stripped and split, as for ctcdec_set_hotwords), weight set_weight[k]; utterance / stream u uses set
 * utt_set[u] (-1: none) in place of the call-wide set and DecodeParams hotword_weight.  A call whose utterance or stream
 * count differs from n_utts fails (CTCDEC_ERR_ARG).  A backend whose kernels do not take per-utterance sets refuses them
 * here (CTCDEC_ERR_LIMIT). */
int ctcdec_set_hotword_sets(ctcdec_decoder* dec, const char* blob, const int64_t* off, int64_t n_words,
                            const int64_t* set_off, int32_t n_sets, const double* set_weight,
                            const int32_t* utt_set, int32_t n_utts);

/* ---- the hot path: replaces decode_beams / decode_batch / decode_beams_batch ------------------
 * utt_logits[i] points to a row-major [utt_frames[i], n_labels] matrix of `dtype`; pointers may
 * be device (HBM-resident, no copy) or host memory (copied H2D first), is_device tells which.
 * start_states may be NULL. The call returns when results are on the host. */
int ctcdec_decode_batch(ctcdec_decoder* dec, const void* const* utt_logits,
                        const int32_t* utt_frames, int32_t n_utts, int32_t dtype, int32_t is_device,
                        const ctcdec_params* params, const ctcdec_lm_state* start_states,
                        ctcdec_result** out);

/* ---- streaming: replaces partial_decode_beams (decoder.py:681-728) for a batch of streams -------
 * Every stream hands back the beams the previous call returned (rank order). Strings travel as
 * byte ranges of text_blob: `text` = completed words separated by single spaces, `partial` = the
 * open partial_word. raw_lm_score / lm_state are the memo values of the text
 * (cached_lm_scores[(text, False)], decoder.py:121-126); (0, LM start state) for the empty text.
 * force_next_word / is_end as in decoder.py:693-694. Results: the packed view incl. its streaming
 * extras; word frames there are only the words closed during THIS call. */
typedef struct ctcdec_beam_in {
  double logit_score;
  double raw_lm_score;
  ctcdec_lm_state lm_state;
  int32_t last_char;          /* label index, -1 = None */
  int32_t partial_start;      /* partial_frames */
  int32_t partial_end_frame;
  int32_t reserved;
  int64_t text_begin, text_end;        /* byte range in text_blob */
  int64_t partial_begin, partial_end;  /* byte range in text_blob */
  const ctcdec_lm_state* more_states;  /* several language models: the states of model 1.. (n-1 entries,
                                          lm_state above being model 0's); NULL with a single model */
} ctcdec_beam_in;
int ctcdec_decode_stream_batch(ctcdec_decoder* dec, const void* const* utt_logits,
                               const int32_t* utt_frames, int32_t n_streams, int32_t dtype,
                               int32_t is_device, const ctcdec_params* params,
                               const int32_t* first_frame /* [n_streams] processed_frames */,
                               const ctcdec_beam_in* beams, const int64_t* beam_off /* [n_streams+1] */,
                               const char* text_blob, int32_t force_next_word, int32_t is_end,
                               ctcdec_result** out);

/* ---- device-resident streams ---------------------------------------------------------------------
 * The same recursion as ctcdec_decode_stream_batch (get_starting_state / partial_decode_beams,
 * decoder.py:669-728), but what the reference's caller carries between chunks -- the live beams, their LM states and
 * memo values, the words and frames decoded so far -- stays on the device: a chunk costs two kernel launches and a
 * 16-byte read-back per stream, and beams are only materialised when somebody asks for them.
 *   open   n independent streams, each at the reference's starting state (start_states: n * max(1, n_lms) LM
 *          states or NULL for the models' own defaults)
 *   push   one chunk per stream (chunk_frames[u] may be 0). first_frame: processed_frames per stream, NULL = the frames
 *          pushed so far. want_result != 0 (always the case for is_end): *out receives the ranked beams exactly as
 *          ctcdec_decode_stream_batch would return them -- texts / word frames from the START of the stream, src_beam = -1
 *          (or, below a ctcdec_stream_import, relative to the imported beam src_beam). After is_end the streams are back
 *          at the starting state.
 *   read   the current beams without advancing (a push of zero frames)
 *   import replace the carried beams of every stream by beams the caller built or edited (the slow path: the host
 *          resolves their strings like ctcdec_decode_stream_batch does). The arrays must stay untouched until close or the
 *          next import (they are copied).
 * One handle belongs to one decoder; its calls are serialised with that decoder's other calls. */
typedef struct ctcdec_stream ctcdec_stream;
/* (tokens and confidences of a stream: below ctcdec_stream_import) */
int ctcdec_stream_open(ctcdec_decoder* dec, int32_t n_streams, const ctcdec_lm_state* start_states, ctcdec_stream** out);
int ctcdec_stream_push(ctcdec_stream* st, const void* const* chunk_logits, const int32_t* chunk_frames, int32_t dtype,
                       int32_t is_device, const ctcdec_params* params, const int32_t* first_frame,
                       int32_t force_next_word, int32_t is_end, int32_t want_result, ctcdec_result** out);
int ctcdec_stream_read(ctcdec_stream* st, const ctcdec_params* params, ctcdec_result** out);
int ctcdec_stream_import(ctcdec_stream* st, const ctcdec_beam_in* beams, const int64_t* beam_off /* [n_streams+1] */,
                         const char* text_blob, int64_t text_bytes);
/* Tokens and confidences (params.token_frames): a stream's emission chains reach back to its start, so a push or read
 * with token_frames = 1 lists the tokens of every word closed so far (a word closed by force_next_word included) and then
 * those of the open partial word, with absolute frames -- at any chunk. A fold (CTCDEC_TOKEN_LOGP_*) needs the per-frame
 * survivors of EARLIER chunks, which the handle then keeps in a device-side ledger (compact, grow-only: a few entries per
 * frame): it has to be asked for by the stream's FIRST push (the first after open or after is_end) and every later push
 * or read may ask for that fold, for token_frames = 1 or for nothing. Such a stream numbers its frames from its first
 * chunk's first_frame: every later first_frame[u] has to equal it plus the frames pushed so far. CTCDEC_ERR_ARG, before
 * the stream is touched: a fold the first push did not ask for (or another one), a first_frame that does not continue the
 * stream, token_frames != 0 on a stream that holds imported beams (their chains start at the import). A streamed token's
 * confidence is the same float64 as ctcdec_decode_batch's for the same frames. */
/* frames pushed so far per stream ([n_streams]) */
int ctcdec_stream_frames(const ctcdec_stream* st, int64_t* frames_out);
/* device bytes the handle's survivor ledger holds (0: no push of it has asked for a confidence fold) */
int ctcdec_stream_ledger_bytes(const ctcdec_stream* st, int64_t* bytes_out);
void ctcdec_stream_close(ctcdec_stream* st);

/* ---- results (OutputBeam fields, decoder.py:102-110, assembled as decoder.py:653-667) --------- */
int32_t ctcdec_result_num_utts(const ctcdec_result* r);
int32_t ctcdec_result_num_beams(const ctcdec_result* r, int32_t utt);
/* text of beam b of utterance u (UTF-8, not NUL-terminated) */
int ctcdec_result_text(const ctcdec_result* r, int32_t utt, int32_t beam, const char** str_out,
                       int64_t* len_out);
int ctcdec_result_scores(const ctcdec_result* r, int32_t utt, int32_t beam, double* logit_score,
                         double* lm_score);
/* word frames: n words; word k spans bytes [word_off[k], word_off[k+1]) of the text and frames
 * [start[k], end[k]). Pointers stay valid until ctcdec_result_free. */
int ctcdec_result_frames(const ctcdec_result* r, int32_t utt, int32_t beam, int32_t* n_words,
                         const int32_t** word_off, const int32_t** start, const int32_t** end);
int ctcdec_result_lm_state(const ctcdec_result* r, int32_t utt, int32_t beam, ctcdec_lm_state* out);
/* several language models: the state of model k (k = 0 is ctcdec_result_lm_state) */
int ctcdec_result_lm_state_of(const ctcdec_result* r, int32_t utt, int32_t beam, int32_t k,
                              ctcdec_lm_state* out);
/* Bulk view of a whole result (one call instead of four per beam): beams of utterance u are
 * [beam_off[u], beam_off[u+1]); beam k's text is text_blob[text_off[k] .. text_off[k+1]); its words
 * are [word_cnt_off[k], word_cnt_off[k+1]) in word_byte_off / word_start / word_end, where
 * word_byte_off is relative to the beam's text and word j ends where word j+1 starts minus one
 * space (or at the end of the text). Pointers stay valid until ctcdec_result_free. */
typedef struct ctcdec_packed {
  int64_t n_utts, n_beams, n_words;
  const int64_t* beam_off;      /* [n_utts + 1]  */
  const char* text_blob;
  const int64_t* text_off;      /* [n_beams + 1] */
  const double* logit_score;    /* [n_beams]     */
  const double* lm_score;       /* [n_beams]     */
  const int64_t* word_cnt_off;  /* [n_beams + 1] */
  const int32_t* word_byte_off; /* [n_words]     */
  const int32_t* word_start;    /* [n_words]     */
  const int32_t* word_end;      /* [n_words]     */
  const ctcdec_lm_state* lm_state; /* [n_beams]  */
  /* streaming extras (LMBeam fields of partial_decode_beams, decoder.py:69-99) */
  const char* partial_blob;        /* still open partial_word of every beam */
  const int64_t* partial_off;      /* [n_beams + 1] */
  const int32_t* src_beam;         /* [n_beams] index of the carried-in beam this beam descends from */
  const int32_t* last_char;        /* [n_beams] label index, -1 = None */
  const int32_t* partial_start;    /* [n_beams] partial_frames */
  const int32_t* partial_end;      /* [n_beams] */
  const double* raw_lm_score;      /* [n_beams] LM score sum of the beam's text (memo value) */
} ctcdec_packed;
int ctcdec_result_pack(ctcdec_result* r, ctcdec_packed* out);
/* Only the texts of all beams (utterance-major, the order of ctcdec_result_pack): UTF-8 blob + n+1 byte offsets. What
 * decode_batch needs (decoder.py:895-945) without packing word frames and states. Owned by the result. */
int ctcdec_result_texts(ctcdec_result* r, const char** blob_out, const int64_t** off_out, int64_t* n_out);
/* The same texts as ONE buffer with `sep` between consecutive texts (n - 1 separators, none at the end): a caller whose
 * language splits strings natively (Python: str.split) gets its n string objects in one call instead of n slices.
 * The caller picks a byte that cannot occur in a text (a label containing it rules this entry point out). */
int ctcdec_result_texts_joined(ctcdec_result* r, char sep, const char** blob_out, int64_t* bytes_out, int64_t* n_out);
/* ... or without any copy: text i is pool[off[i] .. off[i] + len[i]) (in whatever order the pool happens to hold them).
 * Pointers stay valid until ctcdec_result_free. */
int ctcdec_result_text_blocks(ctcdec_result* r, const char** pool_out, const int64_t** off_out, const int64_t** len_out,
                              int64_t* n_out);

/* Per-token frames of every beam of a result decoded with params.token_frames = 1, in the order of ctcdec_result_pack:
 * beam k's tokens are [tok_off[k], tok_off[k+1]) (tok_off has n_beams + 1 entries) in label / start / end. A token is a
 * non-blank emission on the beam's path that is not a space label of a character alphabet: label is its alphabet index,
 * start the absolute frame at which the beam took it after a blank or another label, end 1 + the last frame of the run
 * of that label which follows it. This is the reference's partial_frames bookkeeping (decoder.py:449-534) applied to one
 * token instead of one word: each word of ctcdec_result_frames is a run of consecutive tokens, from its first token's
 * start to its last token's end. A device-resident stream (ctcdec_stream_push / _read) lists the tokens from the start of
 * the stream, the open partial word's last; ctcdec_decode_stream_batch lists only the tokens decoded on the device since
 * the caller's beams were imported. Pointers stay valid until ctcdec_result_free; a result
 * decoded without params.token_frames returns CTCDEC_ERR_ARG. */
int ctcdec_result_token_frames(ctcdec_result* r, const int64_t** tok_off, const int32_t** label, const int32_t** start,
                               const int32_t** end, int64_t* n_tokens);

/* Per-token confidences of a result decoded with params.token_frames = CTCDEC_TOKEN_LOGP_MEAN / _MIN / _MAX, in the order
 * of ctcdec_result_token_frames (n_tokens is the same): logp[i] folds, over the frames [start, end) of token i, the natural-log
 * probability of the token's label at that frame -- the clipped log-softmax (or log(clip(p))) the token prune looked at
 * (decoder.py:180-197, 444-445, 762-765) -- as the arithmetic mean (summed in frame order; the log of the geometric mean), the
 * minimum or the maximum. The values are computed on the device inside the decode call, from the survivor lists of its
 * frame-prune stage: a token's label survived the prune at every frame of its run. A device-resident stream folds over its
 * survivor ledger instead, which holds the same values for every frame pushed so far (ctcdec_stream_push). Pointers stay
 * valid until ctcdec_result_free; a result decoded without a fold returns CTCDEC_ERR_ARG, and ctcdec_decode_stream_batch
 * refuses the fold. decode_beams(..., confidence="mean") / decode_batch / partial_decode_beams(..., confidence=...) */
int ctcdec_result_token_logp(ctcdec_result* r, const double** logp, int64_t* n_tokens);

/* ---- forced alignment: where a transcript the caller already has lies in the audio ---------------------------------
 * No reference analogue (pyctcdecode decodes; torchaudio.functional.forced_align is the usual tool). Utterance u's target
 * is the label ids targets[target_off[u] .. target_off[u + 1]) (alphabet indices, never the blank; at most 2047 of them);
 * logits, frame counts, dtype and is_device are those of ctcdec_decode_batch, and the probabilities-or-logits rule is the
 * decode's own (the same device-side test). The library finds the path through blank / label / blank / ... that maximises the
 * sum of the frames' log-probabilities -- clip(log_softmax(x), ln 1e-15, 0), or log(clip(p, 1e-15, 1)) of probability-like
 * input, all in float64 (every input dtype widens exactly; the float32 prune path's bits are not reproduced). Equal scores
 * prefer staying in a state, then the next state, then the skip over a blank; the last label is preferred over a trailing blank.
 * fold: 0, or CTCDEC_TOKEN_LOGP_MEAN / _MIN / _MAX for each target label's confidence over its own frames of the path.
 * bp_budget: bytes of back-pointer tables (frames * ceil((2 L + 1) / 4) per utterance) one kernel launch may hold, 0 for the
 * default of 1 GiB; a batch that needs more is aligned in several launches with the same results.
 * Everything is validated before anything is launched: a label outside the alphabet or equal to the blank, or an utterance
 * with fewer frames than labels plus adjacent equal labels (no path exists; the message lists the utterances) is
 * CTCDEC_ERR_ARG; more than 2047 labels, or one utterance whose table alone exceeds the budget, is CTCDEC_ERR_LIMIT.
 * Text-to-label mapping and word grouping are the caller's (decoder.py: align / align_batch). */
typedef struct ctcdec_alignment ctcdec_alignment; /* opaque */
int ctcdec_align_batch(ctcdec_decoder* dec, const void* const* utt_logits, const int32_t* utt_frames, int32_t n_utts,
                       int32_t dtype, int32_t is_device, const int32_t* targets, const int64_t* target_off, int32_t fold,
                       int64_t bp_budget, ctcdec_alignment** out);
/* Utterance u's path is path[path_off[u] .. path_off[u + 1]): the label taken at each frame, the blank's index for blanks;
 * score[u] is the sum of the log-probabilities along it. Pointers stay valid until ctcdec_alignment_free. */
int ctcdec_alignment_paths(const ctcdec_alignment* a, const int64_t** path_off, const int32_t** path, const double** score,
                           int64_t* n_utts);
/* Every target label with its frames, in the layout of ctcdec_result_token_frames / ctcdec_result_token_logp: utterance u's
 * are [tok_off[u], tok_off[u + 1]) of label / start / end (end exclusive) and, when a fold was asked for, logp (else NULL). */
int ctcdec_alignment_tokens(const ctcdec_alignment* a, const int64_t** tok_off, const int32_t** label, const int32_t** start,
                            const int32_t** end, const double** logp, int64_t* n_tokens);
/* milliseconds: [0] the classification (frame-prune kernels), [1] row_lse, [2] ctc_viterbi (HIP events on the decode
 * stream, summed over the launches), [3] the whole native call; launches: ctc_viterbi launches the budget made (may be NULL) */
int ctcdec_alignment_timing(const ctcdec_alignment* a, double* ms4, int32_t* launches);
void ctcdec_alignment_free(ctcdec_alignment* a);

/* ---- forced alignment of long transcripts: a lecture against its script ------------------------------------------------
 * ctcdec_align_batch without its two limits: at most 1048575 labels per utterance (2 L + 1 states below 2^21) instead of
 * 2047, and no back-pointer table of all frames. For every input ctcdec_align_batch accepts the result is that call's, bit
 * for bit -- path, score, token frames and confidences --, however the frames are cut: the recursion, its operands, their
 * order and the tie rules are the same. Both score columns live in device memory (kernel ctc_viterbi_long, one workgroup
 * per utterance), so for short targets ctcdec_align_batch is the faster call.
 * The frames 1 .. T - 1 of an utterance are cut into n = ceil((T - 1) / K) segments of K frames. With nch = ceil((2 L + 1) / 4)
 * its plan takes  K * nch + (n > 1 ? 32 * nch * n : 0) + 64 * nch  bytes: one segment's back-pointers, the score column every
 * segment starts from, the two columns. One segment is one pass, as ctcdec_align_batch makes it; more segments are one pass
 * that keeps the checkpoints and a second, from the last segment to the first, that fills and traces back one table each.
 * segment_frames: 0 -- one segment (K = T) when that plan fits the budget, else K = min(T, ceil(sqrt(32 T))) --, or > 0 to
 * force K = min(segment_frames, T). bp_budget: the planned bytes one launch may hold, 0 for 1 GiB; a batch that needs more is
 * aligned in several launches with the same results.
 * Validation, before any launch: ctcdec_align_batch's checks with its codes; segment_frames < 0 is CTCDEC_ERR_ARG; more than
 * 1048575 labels, or one utterance whose plan exceeds the budget, is CTCDEC_ERR_LIMIT and names the utterance.
 * The result is read by ctcdec_alignment_paths / _tokens / _timing ([2] ctc_viterbi_long) / _plan and freed by
 * ctcdec_alignment_free. decoder.py: align_long / align_long_batch. */
int ctcdec_align_long_batch(ctcdec_decoder* dec, const void* const* utt_logits, const int32_t* utt_frames, int32_t n_utts,
                            int32_t dtype, int32_t is_device, const int32_t* targets, const int64_t* target_off, int32_t fold,
                            int64_t bp_budget, int32_t segment_frames, ctcdec_alignment** out);
/* How each utterance's frames were cut: segment_frames[u] = K and n_segments[u] = ceil((T - 1) / K) (0 / 0 without frames). An
 * alignment made by ctcdec_align_batch or ctcdec_align_gaps_batch reports one segment of all T frames. */
int ctcdec_alignment_plan(const ctcdec_alignment* a, const int32_t** segment_frames, const int32_t** n_segments, int64_t* n_utts);

/* ---- alignment with gaps: a transcript that does not cover all of the audio ------------------------------------------
 * torchaudio's forced_align tutorials do this with a "star" token. ctcdec_align_batch with one more kind of target item:
 * CTCDEC_ALIGN_GAP stands for "something nobody transcribed". A target is a sequence of items, each a label id (alphabet
 * index, never the blank) or a gap; with L labels y[0 .. L) there are L + 1 slots -- before y[0], between neighbours, after
 * y[L - 1] --, each plain or a gap. The states are ctcdec_align_batch's, S = 2 L + 1: even state 2 j is slot j, odd state
 * 2 k + 1 is label k. With e(t, c) that call's clipped float64 log-probabilities:
 *   a label state emits e(t, y[k]); a plain slot emits e(t, blank);
 *   a gap slot emits g(t), the largest e(t, c) over all columns c, the blank included -- the clipped value of the row's
 *   largest entry that is not a NaN (a row without one takes the floor, as every NaN entry does).
 * So a gap is a blank that may also absorb any labels, at the price the best unconstrained path would pay for those frames.
 * It may be empty wherever the plain blank may be skipped; between two equal labels it takes at least one frame, as the
 * blank does. Transitions are unchanged: stay, step, and the skip for a label that differs from the label before it.
 * Ties: in label states and plain slots equal scores prefer stay, then step, then skip; in a gap slot they prefer step over
 * stay. (Wherever a target label is its row's maximum, g(t) equals e(t, label) bit for bit, and "the label keeps this frame"
 * ties with "the gap already has it": under this rule such frames go to the label at both of its ends.) At the end the last
 * label is preferred over the trailing slot. A path exists when T >= L + (adjacent equal labels); a target needs a label.
 * Two consequences are exact, because floating-point addition is monotone and the sums run in frame order: a target without
 * gaps gives ctcdec_align_batch's path, token frames, confidences and score, bit for bit; the score with gaps is >= that
 * call's score for the same labels and <= the sum of g(t) over all frames.
 * The arguments are ctcdec_align_batch's, except that targets may hold CTCDEC_ALIGN_GAP. Validation, before any launch:
 * that call's checks with its codes (on the labels alone: gaps do not count towards the 2047); two adjacent gaps or a target
 * without a label is CTCDEC_ERR_ARG. The budget is that call's (the tables are as large).
 * The result is read by ctcdec_alignment_paths (path holds -1 on the frames spent in a gap slot), ctcdec_alignment_tokens
 * (labels only), ctcdec_alignment_timing ([1] row_lse_max, [2] ctc_viterbi_gaps) and ctcdec_alignment_gaps, and freed by
 * ctcdec_alignment_free. decoder.py: align_gaps / align_gaps_batch. */
#define CTCDEC_ALIGN_GAP (-1)
int ctcdec_align_gaps_batch(ctcdec_decoder* dec, const void* const* utt_logits, const int32_t* utt_frames, int32_t n_utts,
                            int32_t dtype, int32_t is_device, const int32_t* targets, const int64_t* target_off, int32_t fold,
                            int64_t bp_budget, ctcdec_alignment** out);
/* Utterance u's gaps, in target order, are [gap_off[u], gap_off[u + 1]) of start / end / logp. A gap's frames [start, end)
 * are everything between the end of the label before it (0 for a leading gap) and the start of the label after it (T for a
 * trailing one): an empty gap has start == end. logp is the sum of g(t) over them, in frame order. CTCDEC_ERR_ARG on an
 * alignment made by ctcdec_align_batch. */
int ctcdec_alignment_gaps(const ctcdec_alignment* a, const int64_t** gap_off, const int32_t** start, const int32_t** end,
                          const double** logp, int64_t* n_gaps);

/* ---- greedy decode: the best path over all texts ----------------------------------------------------------------------
 * No reference analogue (pyctcdecode always searches). Logits, frame counts, dtype and is_device are those of
 * ctcdec_decode_batch. Frame t's label arg[t] is the smallest index among the entries of row t that equal the row's largest
 * entry that is not a NaN (-0.0 and +0.0 are equal; a row without an entry above -inf takes the blank): the same for logits
 * and for probabilities, so nothing is classified. A token is a maximal run of frames with the same label other than the
 * blank: (label, start, end), end exclusive; equal labels with a blank frame between them are two tokens; an utterance has at
 * most as many tokens as frames, and none of ctcdec_align_batch's limits applies. The text of an utterance is formed from
 * its tokens' labels on the host: under a character alphabet the space label ends a word (it is a token of the result all
 * the same), under a BPE alphabet a leading U+2581 begins a word and a trailing one ends it; words are joined by one space.
 * fold: 0 -- one kernel reads every entry once and compares, a second collapses the labels: no classification, no
 * exponential --, or CTCDEC_TOKEN_LOGP_MEAN / _MIN / _MAX. With a fold the call classifies as ctcdec_align_batch does and
 * forms e(t), ctcdec_align_gaps_batch's g(t): the clipped float64 log-probability of row t's largest entry. score[u] is the
 * sum of e(t) over all of utterance u's frames, blanks included, added in frame order; a token's logp is the fold of e(t)
 * over its frames, in frame order. Both sums run as ctcdec_align_batch's do, so for an utterance with a token score[u]
 * equals, bit for bit, that call's score for the greedy labels as the target -- no path beats the frames' maxima -- and that
 * of ctcdec_align_gaps_batch with every slot a gap.
 * CTCDEC_ERR_ARG before anything is launched: a null pointer, a negative frame count, a bad dtype or fold. Without frames
 * nothing is launched. decoder.py: decode_greedy / decode_greedy_batch. */
typedef struct ctcdec_greedy ctcdec_greedy; /* opaque */
int ctcdec_greedy_batch(ctcdec_decoder* dec, const void* const* utt_logits, const int32_t* utt_frames, int32_t n_utts,
                        int32_t dtype, int32_t is_device, int32_t fold, ctcdec_greedy** out);
/* Utterance u's text is the UTF-8 bytes blob[off[u] .. off[u + 1]). Pointers stay valid until ctcdec_greedy_free. */
int ctcdec_greedy_texts(const ctcdec_greedy* g, const char** blob, const int64_t** off, int64_t* n_utts);
/* Every token, in the layout of ctcdec_alignment_tokens: utterance u's are [tok_off[u], tok_off[u + 1]) of label / start /
 * end (end exclusive) and, when a fold was asked for, logp (else NULL). */
int ctcdec_greedy_tokens(const ctcdec_greedy* g, const int64_t** tok_off, const int32_t** label, const int32_t** start,
                         const int32_t** end, const double** logp, int64_t* n_tokens);
/* score[u]: the sum of e(t) over utterance u's frames (0.0 without frames); NULL when no fold was asked for */
int ctcdec_greedy_scores(const ctcdec_greedy* g, const double** score, int64_t* n_utts);
/* milliseconds: [0] the classification (frame-prune kernels; 0 without a fold), [1] the row kernel -- row_argmax, or
 * row_lse_argmax with a fold --, [2] greedy_collapse's two passes (HIP events on the decode stream), [3] the whole native
 * call; launches: kernels launched after the classification (may be NULL); lse_ms: the part of [1] that a kernel with a
 * log-sum-exp took -- [1] with a fold, 0 without (may be NULL) */
int ctcdec_greedy_timing(const ctcdec_greedy* g, double* ms4, int32_t* launches, double* lse_ms);
void ctcdec_greedy_free(ctcdec_greedy* g);

/* ---- transcript likelihood: how probable a label sequence the caller already has is, given the audio -----------------
 * No reference analogue (torch.nn.functional.ctc_loss computes the negative of it). Utterance u owns the hypotheses
 * [hyp_off[u], hyp_off[u + 1]); hypothesis h is the label ids targets[target_off[h] .. target_off[h + 1]) (alphabet
 * indices, never the blank; at most 2047 of them). Logits, frame counts, dtype, is_device, the probabilities-or-logits
 * rule and the per-frame log-probabilities (clipped, float64) are those of ctcdec_align_batch. logp_out[h] is the CTC forward
 * score: the natural log of the sum, over ALL paths through blank / label / blank / ... that collapse to the hypothesis,
 * of the product of the frames' probabilities -- where ctcdec_align_batch's score is the largest single term of that sum.
 * Each step adds its two or three predecessors as m + log(sum of exp(v - m)) in float64. A hypothesis with fewer frames
 * than labels plus adjacent equal labels has no path: -inf (decided by the host; not an error). The empty hypothesis scores
 * the all-blank path, and 0.0 for an utterance without frames. The row log-sum-exps are computed once per utterance,
 * however many hypotheses it has; an utterance none of whose hypotheses is launched (none given, or none with a path) is
 * neither staged nor classified nor summed.
 * kernel: 0 lets the library choose between its two kernels (one wavefront per hypothesis up to 127 labels, one workgroup
 * above), 1 prefers the wavefront kernel (longer hypotheses still take the workgroup kernel), 2 forces the workgroup kernel;
 * both return the same bits. score / score_batch pass it from the environment variable CTCDEC_FORWARD_KERNEL=wave|group.
 * ms4 (may be NULL): milliseconds of [0] the classification, [1] row_lse, [2] the forward kernels (HIP events on the decode
 * stream), [3] the whole native call. launched2 (may be NULL): hypotheses that went to [0] the wavefront kernel, [1] the
 * workgroup kernel. Everything is validated before anything is launched: a null pointer, offsets that do not start at 0 or
 * decrease, a negative frame count, a label outside the alphabet or equal to the blank is CTCDEC_ERR_ARG; more than 2047
 * labels is CTCDEC_ERR_LIMIT. Text-to-label mapping and the language-model term are the caller's (decoder.py: score /
 * score_batch). */
int ctcdec_score_batch(ctcdec_decoder* dec, const void* const* utt_logits, const int32_t* utt_frames, int32_t n_utts,
                       int32_t dtype, int32_t is_device, const int32_t* targets, const int64_t* target_off,
                       const int64_t* hyp_off, int32_t kernel, double* logp_out, double* ms4, int64_t* launched2);

/* ---- prefix scores: how probable it is that the transcript STARTS with a label sequence followed by label c, for every c ---
 * No reference analogue: the CTC prefix score an external decoder asks for at every step (joint CTC / attention decoding,
 * rescoring another model's next-token distribution, constrained decoding). Utterance u owns the prefixes
 * [prefix_off[u], prefix_off[u + 1]); prefix h is the label ids labels[label_off[h] .. label_off[h + 1]) (alphabet indices,
 * never the blank; at most 2047 of them; none: the empty prefix). Logits, frame counts, dtype, is_device, the
 * probabilities-or-logits rule and the per-frame log-probabilities e(t, c) (clipped, float64) are those of
 * ctcdec_align_batch; a_t[s] is ctcdec_score_batch's forward recursion over the S = 2 L + 1 states of the prefix. With
 *   B[0] = -inf,  B[t >= 1] = a_{t-1}[S-1],
 *   A[0] = 0 for the empty prefix, else -inf,  A[t >= 1] = lse2(a_{t-1}[S-1], a_{t-1}[S-2])  (L = 0: a_{t-1}[0]),
 *   end[h]      = lse2(a_{T-1}[S-1], a_{T-1}[S-2]): ctcdec_score_batch's score of the prefix as a whole transcript, bit for bit;
 *   next[h][c]  = log sum_t exp(W_c[t] + e(t, c)),  W_c = B when c is the prefix' last label, else A;  next[h][blank] = -inf:
 * the mass of all frame sequences whose labels through some frame t are exactly the prefix and then c, c first completed
 * at t -- for normalised rows the probability that the transcript starts with the prefix followed by c. A prefix with
 * fewer frames than labels plus adjacent equal labels has end = -inf and next = -inf everywhere and launches nothing; with
 * exactly as many, end is finite and next all -inf; without frames the empty prefix has end = 0.0.
 * The call is stateless: each prefix' forward pass runs from scratch (ctc_forward / ctc_forward_wave with per-frame end
 * states; `kernel` as in ctcdec_score_batch, the same bits either way), then ctc_prefix_extend forms all V scores of up to 8
 * prefixes of an utterance from one read of its rows. The row log-sum-exps are computed once per utterance. No atomics:
 * a prefix' bits do not depend on the rest of the batch or on host / device input.
 * next_out: NULL -- the result holds next as one [n_prefixes][V] float64 block --, or (is_device only) device memory of
 * that shape, which the kernels write in place; the call returns when they have.
 * Everything is validated before anything is launched, as in ctcdec_score_batch (CTCDEC_ERR_ARG; more than 2047 labels:
 * CTCDEC_ERR_LIMIT). decoder.py: prefix_scores / prefix_scores_batch. */
typedef struct ctcdec_prefix ctcdec_prefix; /* opaque */
int ctcdec_prefix_batch(ctcdec_decoder* dec, const void* const* utt_logits, const int32_t* utt_frames, int32_t n_utts,
                        int32_t dtype, int32_t is_device, const int32_t* labels, const int64_t* label_off,
                        const int64_t* prefix_off, int32_t kernel, double* next_out, ctcdec_prefix** out);
/* end[n_prefixes]; next[n_prefixes * n_labels], NULL when the call was given next_out. Valid until ctcdec_prefix_free. */
int ctcdec_prefix_scores(const ctcdec_prefix* p, const double** end, const double** next, int64_t* n_prefixes, int32_t* n_labels);
/* milliseconds: [0] the classification, [1] row_lse, [2] the forward kernels with end states, [3] ctc_prefix_extend (with
 * ctc_prefix_finish and the fill of rows without a launch; HIP events on the decode stream), [4] the whole native call;
 * launches3 (may be NULL): kernel launches of [0] row_lse -- one, however many prefixes an utterance has --, [1] the forward
 * kernels, [2] ctc_prefix_extend, ctc_prefix_finish and the fill, as the kernels' event logs counted them; launched2 (may
 * be NULL): prefixes that went to [0] the wavefront kernel, [1] the workgroup kernel */
int ctcdec_prefix_timing(const ctcdec_prefix* p, double* ms5, int32_t* launches3, int64_t* launched2);
void ctcdec_prefix_free(ctcdec_prefix* p);

/* ---- prefix sessions: ctcdec_prefix_batch for a decoding loop -- a prefix is extended by one label in O(T) ---------------
 * A decoding loop's prefixes are each a parent of the step before plus one label. A session keeps, per live prefix, what
 * ctcdec_prefix_batch's forward pass leaves behind for it -- bc[t] = a_{t-1}[S-1], bc[T + t] = a_{t-1}[S-2] and their
 * maximum, `scale` -- in a slot of an arena, and forms the child g + [c] from the slot of g alone, by a recursion over the
 * child's two new states, its last label y and its final blank z:
 *   y_0 = e(0, c) for the empty g, else -inf;   z_0 = -inf;
 *   y_t = lse3(y_{t-1}, bc_g[t], c != last(g) ? bc_g[T + t] : -inf) + e(t, c),    z_t = lse2(z_{t-1}, y_{t-1}) + e(t, blank),
 *   bc[t] = z_{t-1},  bc[T + t] = y_{t-1},  end = lse2(z_{T-1}, y_{T-1})
 * (kernel ctc_prefix_advance, one launch per extend), followed by ctcdec_prefix_batch's own ctc_prefix_extend over the new
 * slots. The recursion applies the forward pass' functions to the forward pass' operands in its order, so end and next of
 * every prefix of a session are, bit for bit, what ctcdec_prefix_batch returns for the same labels on the same input. The
 * classification and the row log-sum-exps are computed once, by ctcdec_prefix_session_open.
 * open: logits, frame counts, dtype and is_device as in ctcdec_prefix_batch. The session copies the row log-sum-exps, the
 * classification and, for host input, the staged matrices into memory of its own; device matrices are read in place by
 * every later extend and have to outlive the session. `capacity` slots (>= n_utts) of 2 * max(T) doubles plus a scale are
 * allocated at once and never grow. Utterance u's empty prefix takes slot u for the session's lifetime: its id goes to
 * root_ids[u], its end to root_end[u], its next to row u of next_out (is_device only: device memory [n_utts][V], written
 * in place) or of next_host (host memory of that shape); exactly one of the two is given.
 * extend: child i is parents[i] followed by labels[i]. Checked before anything is launched or taken: every parent a live
 * id of this session, every label inside the alphabet and not the blank (CTCDEC_ERR_ARG), no child longer than 2047
 * labels and n free slots (CTCDEC_ERR_LIMIT; the session is unchanged and usable). A parent may appear any number of
 * times; the ids of a call's children come back with the call, so none of them can be a parent in it. ids_out[n],
 * end_out[n], and next as for open, [n][V]. A child with fewer frames than labels plus adjacent equal labels has end and
 * next of -inf throughout, as in ctcdec_prefix_batch.
 * release: the slots of the ids become free; an id stays dead when its slot is handed out again. Releasing an empty
 * prefix, a dead id or one id twice is CTCDEC_ERR_ARG, and nothing is released. A prefix stays usable as a parent until it
 * is released, whatever became of its own parent.
 * timing, of the last open or extend: ms3 = [0] ctc_prefix_advance, [1] ctc_prefix_extend with ctc_prefix_finish and the
 * fill (HIP events on the decode stream), [2] the whole native call; launches4 (may be NULL) = kernel launches of [0]
 * ctc_prefix_advance, [1] ctc_prefix_extend, ctc_prefix_finish and the fill, [2] row_lse, [3] the forward kernels -- the
 * last two are 0 for an extend.
 * Every entry takes the device lock. The decoder has to outlive its sessions. decoder.py: prefix_session. */
typedef struct ctcdec_prefix_session ctcdec_prefix_session; /* opaque */
int ctcdec_prefix_session_open(ctcdec_decoder* dec, const void* const* utt_logits, const int32_t* utt_frames, int32_t n_utts,
                               int32_t dtype, int32_t is_device, int64_t capacity, double* next_out, int64_t* root_ids,
                               double* root_end, double* next_host, ctcdec_prefix_session** out);
int ctcdec_prefix_session_extend(ctcdec_prefix_session* s, const int64_t* parents, const int32_t* labels, int64_t n,
                                 double* next_out, int64_t* ids_out, double* end_out, double* next_host);
int ctcdec_prefix_session_release(ctcdec_prefix_session* s, const int64_t* ids, int64_t n);
int ctcdec_prefix_session_timing(const ctcdec_prefix_session* s, double* ms3, int32_t* launches4);
void ctcdec_prefix_session_close(ctcdec_prefix_session* s);

/* ---- frame posteriors: where, under ALL alignments of a label sequence the caller already has, each frame lies ---------
 * No reference analogue: the CTC forward-backward. Utterance u's target is labels[label_off[u] .. label_off[u + 1]) (alphabet
 * indices, never the blank; at most 2047 of them); logits, frame counts, dtype, is_device, the probabilities-or-logits rule
 * and the per-frame log-probabilities e(t, s) (clipped, float64) are those of ctcdec_align_batch. Over the S = 2 L + 1 states
 * blank / label 0 / blank / ... / label L - 1 / blank:
 *   a_t[s]: the forward recursion of ctcdec_score_batch, which includes frame t's emission; logp = lse2(a_{T-1}[S-1],
 *           a_{T-1}[S-2]) is that call's score for the same input, bit for bit;
 *   b_t[s]: the log of the sum over all completions from state s after frame t (frame t's emission excluded):
 *           b_{T-1}[S-1] = b_{T-1}[S-2] = 0,
 *           b_t[s] = lse3(b_{t+1}[s] + e(t+1, s), b_{t+1}[s+1] + e(t+1, s+1), skip(s+2) ? b_{t+1}[s+2] + e(t+1, s+2) : -inf),
 *           summed in that order as m + log(sum of exp(v - m));
 *   logp_backward = lse2(b_0[0] + e(0, blank), b_0[1] + e(0, label 0)): logp again, read off the other end;
 *   gamma[t, s] = exp(a_t[s] + b_t[s] - logp), as computed (not clamped: a value may exceed 1 by rounding), and exactly 0.0
 *           for a state outside the window S - 2 - 2 (T - 1 - t) <= s <= 2 t + 1 no alignment passes through;
 *   occupancy[k] = sum over t of gamma[t, 2 k + 1], centre[k] = sum over t of t * gamma[t, 2 k + 1], over occupancy[k]; both
 *           are summed on the device in the order t = T - 1 .. 0 and have the same bits with and without `dense`.
 * dense != 0 also returns gamma (copied to the host launch by launch; 32 * T * ceil(S / 4) bytes per utterance: large batches
 * want dense == 0). table_budget: bytes of such tables one kernel launch may hold, 0 for the default of 4 GiB; a batch that
 * needs more runs in several launches with the same results. Everything is validated before anything is launched, with
 * ctcdec_align_batch's codes: a label outside the alphabet or equal to the blank, or an utterance with fewer frames than
 * labels plus adjacent equal labels (the message lists them) is CTCDEC_ERR_ARG; more than 2047 labels, or one utterance whose
 * table alone exceeds the budget, is CTCDEC_ERR_LIMIT. An utterance without frames and with the empty target has logp 0.0. */
typedef struct ctcdec_posteriors ctcdec_posteriors; /* opaque */
int ctcdec_posteriors_batch(ctcdec_decoder* dec, const void* const* utt_logits, const int32_t* utt_frames, int32_t n_utts,
                            int32_t dtype, int32_t is_device, const int64_t* label_off, const int32_t* labels, int32_t dense,
                            int64_t table_budget, ctcdec_posteriors** out);
/* logp[u] and logp_backward[u] of every utterance. Pointers stay valid until ctcdec_posteriors_free. */
int ctcdec_posteriors_scores(const ctcdec_posteriors* p, const double** logp, const double** logp_backward, int64_t* n_utts);
/* Utterance u's token summaries are [tok_off[u], tok_off[u + 1]) of occupancy / centre (tok_off is label_off). */
int ctcdec_posteriors_tokens(const ctcdec_posteriors* p, const int64_t** tok_off, const double** occupancy, const double** centre,
                             int64_t* n_tokens);
/* The dense tables: utterance u's gamma[t, s] is gamma[gamma_off[u] + t * row_stride[u] + s], s < 2 L + 1 (the row stride, in
 * doubles, is S rounded up to a multiple of four; the padding holds 0.0). gamma is NULL when dense was 0. */
int ctcdec_posteriors_gamma(const ctcdec_posteriors* p, const int64_t** gamma_off, const int32_t** row_stride, const double** gamma);
/* milliseconds: [0] the classification (frame-prune kernels), [1] row_lse, [2] ctc_posteriors (HIP events on the decode
 * stream, summed over the launches), [3] the whole native call; launches: kernel launches made (may be NULL); launched2 (may
 * be NULL): utterances that went to [0] the 256-thread kernel (up to 511 labels), [1] the 1024-thread kernel */
int ctcdec_posteriors_timing(const ctcdec_posteriors* p, double* ms4, int32_t* launches, int64_t* launched2);
void ctcdec_posteriors_free(ctcdec_posteriors* p);

/* ---- transcript gradient: d logp / d (the utterance's own matrix) of a label sequence the caller already has --------------
 * Arguments, checks, codes and messages are those of ctcdec_posteriors_batch; logp_out[u] is its logp[u], bit for bit. With
 * gamma of "frame posteriors", G[t, k] the sum of gamma[t, s] over the states s whose label is k (the blank: the even states),
 * lse[t] the row's log-sum-exp and y = x[t, k] - lse[t]:
 *   logits:        u = y >= ln 1e-15 ? 1 : 0 (a NaN or -inf entry: 0),  G' = u G,  M[t] = sum over k of G'[t, k],
 *                  grad[t, v] = G'[t, v] - exp(x[t, v] - lse[t]) M[t]    (nothing clipped: G - softmax)
 *   probabilities: grad[t, v] = 1e-15 <= p <= 1 ? G[t, v] / p : 0
 * grad_out[u] points to T_u * V elements of grad_dtype -- CTCDEC_F64 for CTCDEC_F64 logits, CTCDEC_F32 for every other dtype;
 * computed in float64 and rounded once -- in host memory when is_device is 0 (the rows are copied back launch by launch), else
 * in device memory, where the kernel writes them in place. An utterance without frames has logp 0.0 and its grad_out[u] is
 * not touched. No floating-point atomics: the same utterance gives the same bits alone and in a batch, in one launch and in
 * several, from host and from device memory. ms5 (may be NULL): [0] the classification, [1] row_lse, [2] ctc_posteriors,
 * [3] ctc_grad_rows (HIP events, summed over the launches), [4] the whole native call; launches (may be NULL): kernel launches
 * of ctc_posteriors and ctc_grad_rows made; launched2 (may be NULL): as ctcdec_posteriors_timing. */
int ctcdec_gradient_batch(ctcdec_decoder* dec, const void* const* utt_logits, const int32_t* utt_frames, int32_t n_utts,
                          int32_t dtype, int32_t is_device, const int64_t* label_off, const int32_t* labels, void* const* grad_out,
                          int32_t grad_dtype, int64_t table_budget, double* logp_out, double* ms5, int32_t* launches,
                          int64_t* launched2);

/* ---- phrase search: does a label sequence occur somewhere in the utterance, where, and how well -------------------------------
 * No reference analogue. Utterance u owns the phrases [hyp_off[u], hyp_off[u + 1]); phrase h is the label ids
 * labels[label_off[h] .. label_off[h + 1]) (alphabet indices, never the blank; 1 to 2047 of them). Logits, frame counts,
 * dtype, is_device, the probabilities-or-logits rule and the per-frame log-probabilities e(t, c) (clipped, float64) are those
 * of ctcdec_align_batch. The states are that call's, S = 2 L + 1, but only the interior states 1 .. S - 2 exist: an
 * occurrence begins on a frame of the first label and ends on a frame of the last. Every state exists in every frame and
 * holds a score d[s] and the frame st[s] its path began on. In frame t state s takes the best of
 *   stay d[s];  step d[s - 1], s >= 2;  skip d[s - 2], s >= 3, a label that differs from the label before it;
 *   a fresh start 0.0 begun at t, for s = 1 alone
 * -- equal scores prefer the earlier in that order --, and adds e(t, label of s); a state with no finite candidate is -inf.
 * After frame t: end_logp[t] = d[S - 2], end_start[t] = st[S - 2] (-inf / -1): the best occurrence whose last label sits on
 * frame t. The hits: until max_hits (1 .. 64) are taken or no end frame qualifies, among the end frames t with a finite
 * end_logp[t] >= min_logp (-inf: no threshold; a NaN is refused) whose window [end_start[t], t] shares no frame with a window
 * taken before, the one with the largest end_logp, the smallest t on a tie. A hit is (start, end = t + 1, logp), in the order
 * taken, best first. An end frame whose best window overlaps a hit already taken is dropped, even if a worse window ending
 * there would not overlap. A phrase with fewer frames than labels plus adjacent equal labels occurs nowhere: no hits, nothing
 * launched (the host decides; not an error), and an utterance none of whose phrases is launched is neither staged nor
 * classified nor summed. want_trace != 0 also returns every phrase's end_logp / end_start rows.
 * kernel: 0 lets the library choose between its two kernels (one wavefront per phrase up to 127 labels, one workgroup above),
 * 1 prefers the wavefront kernel (longer phrases still take the workgroup kernel), 2 forces the workgroup kernel; both return
 * the same bits. find / find_batch pass it from the environment variable CTCDEC_FIND_KERNEL=wave|group.
 * trace_budget: bytes of traces (12 per frame of a launched phrase) one launch may hold, 0 for the default of 1 GiB; a batch
 * that needs more runs in several launches with the same results. Everything is validated before anything is launched: a
 * null pointer, offsets that do not start at 0 or decrease, a negative frame count, a label outside the alphabet or equal to
 * the blank, an empty phrase, max_hits outside 1 .. 64 or a NaN min_logp is CTCDEC_ERR_ARG; more than 2047 labels, or one
 * phrase whose trace alone exceeds the budget, is CTCDEC_ERR_LIMIT. */
typedef struct ctcdec_search ctcdec_search; /* opaque */
int ctcdec_find_batch(ctcdec_decoder* dec, const void* const* utt_logits, const int32_t* utt_frames, int32_t n_utts, int32_t dtype,
                      int32_t is_device, const int64_t* hyp_off, const int64_t* label_off, const int32_t* labels, int32_t max_hits,
                      double min_logp, int32_t want_trace, int32_t kernel, int64_t trace_budget, ctcdec_search** out);
/* Phrase h's hits are [hit_off[h], hit_off[h + 1]) of start / end / logp (its hit count: the difference), best first.
 * Pointers stay valid until ctcdec_search_free. */
int ctcdec_search_hits(const ctcdec_search* s, const int64_t** hit_off, const int32_t** start, const int32_t** end,
                       const double** logp, int64_t* n_phrases);
/* Phrase h's trace is [trace_off[h], trace_off[h + 1]) of end_logp / end_start, one entry per frame of its utterance (-inf /
 * -1 throughout for a phrase that was not launched). Both are NULL, and trace_off all 0, when want_trace was 0. */
int ctcdec_search_trace(const ctcdec_search* s, const int64_t** trace_off, const double** end_logp, const int32_t** end_start);
/* milliseconds: [0] the classification (frame-prune kernels), [1] row_lse, [2] the find kernels (HIP events on the decode
 * stream, summed over the launches), [3] the whole native call; launches: kernel launches made (may be NULL); launched2 (may
 * be NULL): phrases that went to [0] the wavefront kernel, [1] the workgroup kernel */
int ctcdec_search_timing(const ctcdec_search* s, double* ms4, int32_t* launches, int64_t* launched2);
void ctcdec_search_free(ctcdec_search* s);

/* timing of the last call's device stages in milliseconds (HIP events on the decode stream):
 * [0] frame-prune kernel, [1] beam kernel, [2] total device time incl. result copy */
int ctcdec_result_timing(const ctcdec_result* r, double* ms3);
/* which beam kernel produced the result: 1 = one wavefront per utterance (csrc/beam_wave.h: one language model
 * or none, beam_width <= 128, at most 480 survivors per frame), 2 = one workgroup per utterance
 * (csrc/beam_core.h: everything else), 0 = empty batch. The environment variable CTCDEC_BEAM_KERNEL=group|wave
 * forces one of them (tests and tuning). */
int ctcdec_result_beam_kernel(const ctcdec_result* r);
/* HIP device index every decoder of this process runs on (-1 before the first ctcdec_create). One process drives one
 * GPU: a ctcdec_create for a different device is refused (CTCDEC_ERR_DEVICE). */
int ctcdec_device(void);
void ctcdec_result_free(ctcdec_result* r);

/* Diagnostics: the frame-prune stage alone on one [n_frames, V] matrix -- per frame the labels
 * `set(np.where(logp >= token_min_logp)[0]) | {argmax}` in CPython's set ITERATION order (the order the
 * reference walks them in, decoder.py:444-447) with their log-probabilities. counts[t] entries of row t are
 * written to ids / logps at t*stride (at most `stride` of them). Lets a test pin the order emulation on
 * CPython itself. */
int ctcdec_frame_survivors(ctcdec_decoder* dec, const void* logits, int32_t n_frames, int32_t dtype,
                           int32_t is_device, double token_min_logp, int32_t stride, int32_t* counts,
                           int32_t* ids, double* logps);

/* Diagnostics: enable/disable per-phase tick accumulation (100 MHz wall clock) for utterance 0 of the
 * following decode calls and read the 24 counters of the last one. Workgroup kernel: 0 load, 1 modes,
 * 2 completions, 3 keys, 4 merge, 5 score, 6 clear, 7 sort, 8 rebuild, 9 rest, 10 finalise (11.. sub-phases).
 * Wave kernel: 0 load + modes, 1 completions, 2 candidate keys, 3 match, 4 fold, 5 score, 6 rank, 7 rebuild,
 * 8 finalise, 9 pool compaction. No reference analogue. */
int ctcdec_profile_phases(ctcdec_decoder* dec, int32_t enable, uint64_t* ticks_out, int32_t n);

const char* ctcdec_last_error(void);
const char* ctcdec_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CTCDEC_H */
