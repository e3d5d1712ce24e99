// backend.h -- the narrow device interface api.cpp and api_transcript.cpp are written against.
//   * pyctcdecode_amd/csrc/backend_hip.hip : the product (MI355X / gfx950 HIP kernels)
//   * tests/sim/backend_sim.cpp            : sequential CPU execution of the same beam_core.h,
//                                            test infrastructure only (never built into the product)
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "beam_core.h"
#include "ctc_align.h"
#include "surv_ledger.h"
#include "token_logp.h"

namespace ctc {
namespace be {

const char* name();
int init(int device, std::string* err);
int bind_thread(std::string* err);  // make the decoder's device current for the calling host thread
int current_device();               // device index all decoders of this process run on (-1: none yet)
void* alloc(size_t bytes, std::string* err);
void release(void* p);
void* alloc_host(size_t bytes, std::string* err);  // page-locked staging memory for result copies
void release_host(void* p);
int h2d(void* dst, const void* src, size_t bytes, std::string* err);
int d2h(void* dst, const void* src, size_t bytes, std::string* err);
int d2d(void* dst, const void* src, size_t bytes, std::string* err);
int zero(void* dst, size_t bytes, std::string* err);
int sync(std::string* err);
// `height` rows of `width` bytes, host (pitch spitch) -> device (pitch dpitch), on the COPY stream (its own non-blocking stream:
// the kernels queued on the decode stream keep running while the host waits here). Returns when the copy has landed.
int h2d_2d_overlapped(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height, std::string* err);
// Every call above except h2d_2d_overlapped, and every launch below, acts on the one decode stream.
// device -> host on the decode stream WITHOUT waiting: `dst` is page-locked memory, valid after the next sync()
int d2h_async(void* dst, const void* src, size_t bytes, std::string* err);
// host -> device on the decode stream WITHOUT waiting: `src` is page-locked memory the caller leaves alone until the stream has passed it
int h2d_async(void* dst, const void* src, size_t bytes, std::string* err);
int cus();  // compute units of the device

// Frame-prune stage: input normalisation (decoder.py:759-765), token prune (decoder.py:444-445)
// and CPython-set ordering of the survivors, for every frame of every utterance.
struct PruneArgs {
  const void* const* utt_logits;  // [n_utts] device pointers to [T_u, V] matrices
  const int64_t* utt_row0;        // [n_utts + 1] prefix sums of T_u (device)
  int32_t n_utts;
  int64_t n_rows;
  int32_t n_labels;
  int32_t dtype;  // ctcdec_dtype
  double token_min_logp;
  int32_t max_surv;
  double* row_sum;       // [n_rows] scratch
  uint32_t* utt_is_prob; // [n_utts] out: 1 when the input looks like probabilities
  uint32_t* surv_cnt;    // [n_rows]
  uint16_t* surv_id;     // [n_rows * max_surv]
  double* surv_lp;       // [n_rows * max_surv]
  uint32_t* overflow;    // [8] ([4]: the survivors of all rows, summed -- utt_sniff; the caller decides small batches' beam kernel
                         //      by the mean per frame) [0]: a row had more than max_surv survivors, [1]: a probability-like utterance exists,
                         // [2]: an utterance is marked 2 in utt_is_prob (its rows sum to about 1: launch_sniff_exact decides)
                         // [3]: device-side counter of slow_rows
  int32_t pass;          // 0: all utterances as logits + row sums + sniff; 1: redo the probability-like ones
  int32_t rows_aligned16; // every utterance base pointer is 16-byte aligned
  int32_t rows_aligned4;  // ... 4-byte aligned (float32 rows read one label at a time)
  int64_t row_base;      // first row of this launch (utt_row0 and the row-indexed arrays are absolute); n_rows rows follow
  uint32_t* slow_rows;   // [n_rows] scratch, or nullptr: rows (relative to row_base) the 64-rows-per-wave kernel hands to the
                         // per-row one; their count is kept in overflow[3]
  uint32_t* utt_side;    // [n_utts] or nullptr (time-sliced host ingest, api.cpp): set to 3 when this launch's rows of the utterance
                         // were classified as probabilities
  double* utt_sum;       // [n_utts] or nullptr (likewise): the row sums of this launch's rows are added to it
  int32_t dense_hint;    // 1: the caller has seen most rows of such input overflow the 64-rows-per-wave kernel (small vocabulary, flat
                         // logits: every label survives) -- go straight to one wave per row
  // set by launch_prune itself:
  int32_t f32_np;        // float32 rows in the reference's own float32 arithmetic (np_f32.h + numpy's summation order): the default;
                         // 0 under CTCDEC_PRUNE_EXP=pk (round 5's packed polynomial, fp64 from there on) / =f64
  const uint8_t* np_prog;  // frame_prune_fast, f32_np: the pairwise tree over the leaf sums of one row as (dst, src) pairs
  const uint16_t* np_leaf; // ... and the leaves as (offset, length) pairs; np_n_leaf of them
  int32_t np_n_leaf;
  int32_t np_uniform8;     // 1, 2, 4 or 8 leaves of 128 labels each (V = 128 .. 1024 in powers of two): the tree is walked in registers
};
int launch_prune(const PruneArgs& a, std::string* err);
// decoder.py:760 in the input dtype and numpy's summation order for the utterances pass 0 marked ambiguous
int launch_sniff_exact(const PruneArgs& a, std::string* err);

// Beam stage: one workgroup per utterance.
struct BeamArgs {
  DeviceTables tables;  // device pointers
  DecodeParams params;
  int32_t n_utts;
  const int64_t* utt_row0;   // [n_utts + 1] (device)
  const uint32_t* surv_cnt;
  const uint16_t* surv_id;
  const double* surv_lp;
  TextNode* text_nodes;      // arena for all utterances
  EmitNode* emit_nodes;
  const uint64_t* text_off;  // [n_utts + 1] node offsets (device)
  const uint64_t* emit_off;  // [n_utts + 1]
  const LmState* start_states;  // [n_utts * max(1, tables.n_lms)] or nullptr
  LmState* out_xstates;         // several LMs: [n_utts * out_stride * (n_lms - 1)], else nullptr
  OutBeam* out;                 // [n_utts * out_stride]
  int32_t out_stride;
  uint32_t* n_out;              // [n_utts]
  uint32_t* status;             // [n_utts]
  EmitNode* tok_pool;
  unsigned long long* tok_pool_head;  // [1]
  unsigned long long tok_pool_cap;
  unsigned long long* prof;  // [N_PROF] phase cycle counters of utterance 0, or nullptr
  const ImportBeam* imports;   // streaming: all utterances' carried-over beams, or nullptr
  const LmState* import_xstates;  // several LMs: [total beams * (n_lms - 1)] their states of LM 1.., else nullptr
  const int64_t* import_off;   // [n_utts + 1] (device)
  const int32_t* first_frames; // [n_utts] processed_frames per utterance (device), or nullptr
  ColdRec* cold;               // [n_utts * 2 * COLD_STRIDE] scratch of the wave kernel
  PoolPay* pay;                // [n_utts * pay_stride] scratch of the wave kernel (nullptr: the decode is not eligible for it)
  uint64_t pay_stride;
  int32_t max_import;          // streaming: the largest number of beams any stream carries in
  // device-resident streams (ctcdec_stream_*), else nullptr / 0: where stream u's finalisation leaves its beams for the
  // next chunk (carry_out + u * carry_stride; several LMs: carry_xstates + u * carry_stride * (n_lms - 1)), its counters
  // (sstate + u: beams carried in, first free node of its emission arena)
  ImportBeam* carry_out;
  LmState* carry_xstates;
  StreamState* sstate;
  int32_t carry_stride;
  int32_t want_out;            // 0: no output records / emission lists for this launch (resident streams between reads)
  // texts assembled on the device (params.texts_only), else nullptr: utterance u writes its text backwards from the end of
  // text_scratch[text_soff[u] .. text_soff[u + 1]) and copies it to a block of text_pool taken from tok_pool_head[1]
  uint8_t* text_scratch;
  const uint64_t* text_soff;   // [n_utts + 1] (device)
  uint8_t* text_pool;
  unsigned long long text_pool_cap;
  const int32_t* order;        // [n_utts] (device) or nullptr: workgroup b decodes utterance order[b] -- longest first, so
                               // that a ragged batch that needs several rounds of resident waves ends evenly (the hardware
                               // hands the next workgroup to the first free slot: longest-processing-time-first scheduling)
  int32_t resident_in;         // 1: `imports` is the carry buffer itself (stream u: imports + u * carry_stride, sstate[u].n_carry
                               // beams; import_xstates likewise), import_off is not used
  int32_t surv_x16;            // 16 x the mean number of survivors per frame of this launch's rows, as the prune stage counted
                               // them (0: not known). Small batches choose their kernel by it (wave_kernel_chosen).
  int64_t total_rows;          // frames of all utterances of this launch
  // wave kernel, set by launch_beam itself:
  unsigned long long* wave_clock;  // diagnostics (CTCDEC_WAVE_TIMES=<file>), else nullptr: [n_utts * 4] per workgroup {start, end of
                               // its wave (100 MHz real-time counter), HW_ID | XCC_ID << 32, frames}
  int32_t prio_mode;           // issue priority of a wave among the waves of its SIMD (beam_wave_hip.hip, WaveGpuCtx::frame_done):
                               // 0 left alone; 1 + k: rotated every 2^k frames; 32: by the frames it still has to decode against
                               // the launch's average (`progress`); 33: likewise, each remaining frame weighed by what a frame of
                               // this utterance is expected to cost (`block_weight`: survivors per frame against the launch's mean)
  unsigned long long* progress;  // [1] frames decoded so far by all waves of the launch (prio_mode 32; zeroed by launch_beam)
  unsigned long long total_frames;
  float inv_n_utts;
  const float* block_weight;   // [n_utts] (prio_mode 33) expected cost of a frame of the utterance workgroup b decodes, relative to
                               // the launch's mean (utt_weigh / utt_place, backend_hip.hip); the same kernels write `order`
  // per-utterance hot words (ctcdec_set_hotword_sets), else nullptr / 0: the call-wide tables.tok_hot / hot / hot_mask and
  // params.hot_weight hold for every utterance. Utterance u (not workgroup u: `order` moves utterances) uses
  // hot_sets[utt_hot[u]]; launch_beam first fills every set's per-label view, hot_sets[k].tok_hot (n_labels entries each)
  const HotSet* hot_sets = nullptr;  // [n_hot_sets] (device)
  const int32_t* utt_hot = nullptr;  // [n_utts] (device), each in [0, n_hot_sets)
  int32_t n_hot_sets = 0;
};
int launch_beam(const BeamArgs& a, std::string* err);
// Will launch_beam run the wave kernel on these arguments (given payload lines)? THE kernel-selection rule, shared by the
// launcher and by the caller that reserves the wave kernel's scratch: eligibility, the carried-in beams, the batch-size
// rule and the CTCDEC_BEAM_KERNEL override. `a.pay` itself is not looked at.
bool wave_kernel_chosen(const BeamArgs& a);
// Is this batch small enough for the choice to depend on the input (then the caller reads the prune stage's survivor count
// before it launches the beam stage -- one small read-back between the two stages)?
bool beam_kernel_depends_on_input(const BeamArgs& a);

// Token confidences (token_logp.h): one lane per token folds the log-probabilities of the token's label over the frames of its
// run, read from the survivor lists of this call's prune stage. `missing` counts the frames whose list does not hold the label.
struct TokenLogpArgs {
  const TokRun* runs;  // [n_tokens] (device)
  int64_t n_tokens;
  int32_t fold;        // LOGP_MEAN / LOGP_MIN / LOGP_MAX
  const uint32_t* surv_cnt;
  const uint16_t* surv_id;
  const double* surv_lp;
  int32_t max_surv;
  double* out;         // [n_tokens] (device)
  uint32_t* missing;   // [1] (device), zeroed by the caller
};
int launch_token_logp(const TokenLogpArgs& a, std::string* err);
double last_token_logp_ms();  // the last launch_token_logp's kernel time (HIP events); waits for the kernel

// A resident stream's survivor ledger (surv_ledger.h). Append: once per push, when the chunk's survivor lists are final, one
// wavefront per stream copies the first min(surv_cnt, max_surv) entries of each of the chunk's rows (utt_row0[u] ..
// utt_row0[u + 1] of the strided arrays) behind the stream's ledger rows led_row0[u] and extends row_off. Stream u's entry
// count after the chunk goes to used_out[u]; a stream that would pass row_cap / ent_cap (the host reserves the chunk's worst
// case: never) writes nothing there and sets *overrun.
struct LedgerAppendArgs {
  int32_t n_streams;
  const int64_t* utt_row0;    // [n_streams + 1] (device)
  const uint32_t* surv_cnt;
  const uint16_t* surv_id;
  const double* surv_lp;
  int32_t max_surv;
  const uint32_t* led_row0;   // [n_streams] (device): ledger rows of each stream before this chunk
  uint64_t* row_off;          // [n_streams * (row_cap + 1)]
  uint16_t* id;               // [n_streams * ent_cap]
  double* lp;                 // [n_streams * ent_cap]
  uint64_t row_cap, ent_cap;  // rows / entries per stream
  uint64_t* used_out;         // [n_streams] (device)
  uint64_t* overrun;          // [1] (device), zeroed when the ledger was made
};
int launch_ledger_append(const LedgerAppendArgs& a, std::string* err);
// Token confidences of a resident stream: launch_token_logp over ledger rows.
struct LedgerLogpArgs {
  const LedgerRun* runs;  // [n_tokens] (device)
  int64_t n_tokens;
  int32_t fold;           // LOGP_MEAN / LOGP_MIN / LOGP_MAX
  const uint64_t* row_off;
  const uint16_t* id;
  const double* lp;
  uint64_t row_cap, ent_cap;
  double* out;            // [n_tokens] (device)
  uint32_t* missing;      // [1] (device), zeroed by the caller
};
int launch_ledger_logp(const LedgerLogpArgs& a, std::string* err);
// the last launch_ledger_append's / launch_ledger_logp's kernel time (HIP events); waits for the kernel
double last_ledger_append_ms();
double last_ledger_logp_ms();

// Forced alignment (ctc_align.h; kernels: ctc_align_hip.hip). row_lse: the fp64 log-sum-exp of every row of the utterances
// the prune stage's sniff did not classify as probabilities (utt_is_prob[u] == 0); lse is indexed like the prune stage's rows.
struct RowLseArgs {
  const void* const* utt_logits;  // [n_utts] (device)
  const int64_t* utt_row0;        // [n_utts + 1] (device)
  const uint32_t* utt_is_prob;    // [n_utts] (device)
  int32_t n_utts;
  int64_t n_rows;
  int32_t n_labels;
  int32_t dtype;  // ctcdec_dtype
  double* lse;    // [n_rows] out
};
int launch_row_lse(const RowLseArgs& a, std::string* err);
// ctc_viterbi: one workgroup per entry of `utts`, all of them validated by the host (AlignUtt)
struct ViterbiArgs {
  const AlignUtt* utts;  // [n_utts] (device)
  int32_t n_utts;
  int32_t n_labels;
  int32_t dtype;
  int32_t blank;
  int32_t fold;        // 0, LOGP_MEAN / LOGP_MIN / LOGP_MAX
  int32_t max_chunks;  // the largest align_chunks(L) of the launch: sizes the two score columns in LDS
  double clip_lo;      // ln(MIN_TOKEN_CLIP_P)
};
int launch_ctc_viterbi(const ViterbiArgs& a, std::string* err);
// ctc_viterbi_long: one workgroup of 1024 threads per entry of `utts`, all of them validated by the host (AlignLongUtt); the
// columns, checkpoints and segment tables the entries name are theirs alone
struct ViterbiLongArgs {
  const AlignLongUtt* utts;  // [n_utts] (device)
  int32_t n_utts;
  int32_t n_labels;
  int32_t dtype;
  int32_t blank;
  int32_t fold;        // 0, LOGP_MEAN / LOGP_MIN / LOGP_MAX
  int32_t pad;
  double clip_lo;      // ln(MIN_TOKEN_CLIP_P)
};
int launch_ctc_viterbi_long(const ViterbiLongArgs& a, std::string* err);
// ctc_forward (wave == 0: one workgroup per entry of `hyps`) / ctc_forward_wave (wave != 0: one wavefront per entry, every
// L <= FORWARD_WAVE_MAX_LABELS), all entries validated by the host (ForwardHyp)
struct ForwardArgs {
  const ForwardHyp* hyps;  // [n_hyps] (device)
  int32_t n_hyps;
  int32_t n_labels;
  int32_t dtype;
  int32_t blank;
  int32_t max_chunks;  // the largest align_chunks(L) of the launch: sizes ctc_forward's two columns in LDS
  int32_t pad;
  double clip_lo;      // ln(MIN_TOKEN_CLIP_P)
};
int launch_ctc_forward(const ForwardArgs& a, int wave, std::string* err);
// ctc_posteriors: one workgroup per entry of `utts`, all of them validated by the host (PostUtt); 256 threads when every
// utterance of the launch has at most 256 groups of states, else 1024
struct PosteriorsArgs {
  const PostUtt* utts;  // [n_utts] (device)
  int32_t n_utts;
  int32_t n_labels;
  int32_t dtype;
  int32_t blank;
  int32_t max_chunks;  // the largest align_chunks(L) of the launch: sizes the columns in LDS
  int32_t dense;       // 1: the tables are left holding gamma (0.0 outside the window); 0: only the scores and the token sums
  double clip_lo;      // ln(MIN_TOKEN_CLIP_P)
};
int launch_ctc_posteriors(const PosteriorsArgs& a, std::string* err);
// ctc_grad_rows: the threads of a workgroup share one row, or 4 or 16 rows of a small vocabulary, of the n_rows rows of the
// entries of `utts` (GradUtt::row_begin ascending from 0), all of them validated by the host; their tables hold the gamma of
// a dense launch_ctc_posteriors queued before this launch
struct GradRowsArgs {
  const GradUtt* utts;  // [n_utts] (device)
  int32_t n_utts;
  int32_t n_labels;
  int64_t n_rows;
  int32_t dtype;
  int32_t grad_dtype;  // ctcdec_dtype of GradUtt::grad: f64 for f64 rows, f32 for every other dtype
  int32_t blank;
  int32_t pad;
  double clip_lo;      // ln(MIN_TOKEN_CLIP_P)
};
int launch_ctc_grad_rows(const GradRowsArgs& a, std::string* err);
// ctc_find (wave == 0: one workgroup per entry of `phrases`) / ctc_find_wave (wave != 0: one wavefront per entry, every
// L <= FIND_WAVE_MAX_LABELS), all entries validated by the host (FindPhrase)
struct FindArgs {
  const FindPhrase* phrases;  // [n_phrases] (device)
  int32_t n_phrases;
  int32_t n_labels;
  int32_t dtype;
  int32_t blank;
  int32_t max_chunks;  // the largest find_chunks(L) of the launch: sizes ctc_find's two columns in LDS
  int32_t max_hits;    // 1 .. FIND_MAX_HITS
  double clip_lo;      // ln(MIN_TOKEN_CLIP_P)
  double min_logp;     // a hit's least score (-inf: none)
};
int launch_ctc_find(const FindArgs& a, int wave, std::string* err);
// Alignment with gaps. row_lse_max: row_lse (the same bits in a.lse) that also stores each row's largest entry that is not a
// NaN in rmax -- for the rows of probability-like utterances too, which get no log-sum-exp. ctc_viterbi_gaps: one workgroup
// per entry of `utts`, all of them validated by the host (GapsUtt); 256 threads when every utterance of the launch has at
// most 256 groups of states, else 1024
int launch_row_lse_max(const RowLseArgs& a, double* rmax, std::string* err);
struct ViterbiGapsArgs {
  const GapsUtt* utts;  // [n_utts] (device)
  int32_t n_utts;
  int32_t n_labels;
  int32_t dtype;
  int32_t blank;
  int32_t fold;        // 0, LOGP_MEAN / LOGP_MIN / LOGP_MAX
  int32_t max_chunks;  // the largest align_chunks(L) of the launch: sizes the two columns in LDS
  double clip_lo;      // ln(MIN_TOKEN_CLIP_P)
};
int launch_ctc_viterbi_gaps(const ViterbiGapsArgs& a, std::string* err);
// Greedy decode. row_argmax: every row's most probable label -- the smallest index of the row's largest entry that is not a
// NaN, `blank` for a row without an entry above -inf -- in arg[n_rows]; utt_is_prob and lse are not used. row_lse_argmax:
// row_lse_max (the same bits in a.lse and rmax) that also stores row_argmax's label. greedy_collapse: one wavefront per
// utterance, a count pass or a write pass (GreedyArgs)
int launch_row_argmax(const RowLseArgs& a, int32_t* arg, int blank, std::string* err);
int launch_row_lse_argmax(const RowLseArgs& a, double* rmax, int32_t* arg, int blank, std::string* err);
int launch_greedy_collapse(const GreedyArgs& a, std::string* err);
// Prefix scores (ctc_align.h, "ctc_prefix_extend"). launch_ctc_forward_ends: launch_ctc_forward whose kernels also store, for
// entry i of `hyps`, the per-frame end states and their scale where ends[i] says (device). launch_ctc_prefix_extend: every
// label's prefix score of the chunks' prefixes from what those kernels stored; a split launch is followed by ctc_prefix_finish.
// launch_ctc_prefix_fill: -inf into the n_rows (at most 65535 a launch) rows `rows` (device) of next[.][V].
int launch_ctc_forward_ends(const ForwardArgs& a, const PrefixEnds* ends, int wave, std::string* err);
int launch_ctc_prefix_extend(const PrefixExtendArgs& a, std::string* err);
int launch_ctc_prefix_fill(double* next, const int32_t* rows, int32_t n_rows, int32_t V, std::string* err);
// Prefix sessions (ctc_align.h, "ctc_prefix_advance"): the end states, scale and end of every child of `kids`, each from its
// parent's end states; all entries validated by the host (PrefixChild), no child's output another's input
int launch_ctc_prefix_advance(const PrefixAdvanceArgs& a, std::string* err);
// kernel times (HIP events) of the launches of one of these kernels since the last reset; waits for the kernels.
// ctc_forward and ctc_forward_wave share a log (with their _ends forms), as do ctc_find and ctc_find_wave, greedy_collapse's
// two passes, and ctc_prefix_extend, ctc_prefix_finish and ctc_prefix_fill; ctc_prefix_advance has its own.
enum AlignKernel {
  K_ROW_LSE, K_VITERBI, K_FORWARD, K_POSTERIORS, K_GRAD_ROWS, K_FIND, K_ROW_LSE_MAX, K_VITERBI_GAPS, K_ROW_ARGMAX, K_ROW_LSE_ARGMAX,
  K_GREEDY_COLLAPSE, K_PREFIX_EXTEND, K_PREFIX_ADVANCE, K_VITERBI_LONG, ALIGN_KERNELS
};
void align_timing_reset();
double align_kernel_ms(AlignKernel kind);
int align_kernel_launches(AlignKernel kind);  // launches logged for the kernel since the last reset

// stage timing (ms) of the last launch_prune / launch_beam pair, measured on the decode stream
void last_timing(double* prune_ms, double* beam_ms);
// the frame-prune kernels of the last launch_prune sequence alone, whether or not a beam launch followed it (last_timing
// reports a pair, and 0 for both until a beam launch has completed it); waits for the kernels
double last_prune_ms();
// which beam kernel the last launch_beam used: 1 = one wave per utterance (beam_wave.h), 2 = one workgroup
// per utterance (beam_core.h), 0 = none yet
int last_beam_kernel();

}  // namespace be
}  // namespace ctc
