// api_transcript.cpp -- the calls of include/ctcdec.h on known transcripts: forced alignment (with and without gaps), greedy
// decode, transcript likelihood, prefix scores and sessions, frame posteriors, transcript gradient, phrase search. Each checks
// its input, runs the device front, launches one or two kernels and copies the results back; the steps they share come first.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "api_internal.h"


struct ctcdec_alignment {
  std::vector<int64_t> path_off, tok_off;
  std::vector<int32_t> path, label, start, end;
  std::vector<double> score, logp;
  bool has_logp = false;
  int32_t launches = 0;
  double ms[4] = {0, 0, 0, 0};
  // how each utterance's frames were cut (ctcdec_alignment_plan): one segment of all of them unless ctcdec_align_long_batch cut
  std::vector<int32_t> seg_frames, n_segs;
  // ctcdec_align_gaps_batch: utterance u's gaps, in target order, are [gap_off[u], gap_off[u + 1])
  bool has_gaps = false;
  std::vector<int64_t> gap_off;
  std::vector<int32_t> gap_start, gap_end;
  std::vector<double> gap_logp;
};

// The back-pointer tables of one ctc_viterbi launch (T * align_chunks(L) bytes per utterance) when the caller names no budget
static const int64_t ALIGN_BP_BUDGET = (int64_t)1 << 30;

// ---- the plan of ctcdec_align_long_batch ("Forced alignment of long transcripts") ----------------------------
// An utterance's frames in segments of K: a table of K rows, a checkpoint per segment when there is more than one, and the two
// score columns. A pure function of (T, L, budget, segment_frames); decoder.py's _align_long_plan is the same rule.
struct LongPlan {
  int32_t K = 0, n_seg = 0;
  int64_t bytes = 0;
};
static LongPlan long_plan_of(int64_t T, int32_t L, int64_t K) {
  const int64_t nch = align_chunks(L), n = align_long_segments((int32_t)T, (int32_t)K);
  return LongPlan{(int32_t)K, (int32_t)n, K * nch + (n > 1 ? 32 * nch * n : 0) + 64 * nch};
}
static int64_t long_balanced_frames(int64_t T) {  // ceil(sqrt(32 T)), at most T
  int64_t K = (int64_t)sqrt(32.0 * (double)T);
  while (K * K < 32 * T) ++K;
  while (K > 1 && (K - 1) * (K - 1) >= 32 * T) --K;
  return std::min(K, T);
}
// segment_frames > 0: that many frames (at most T); else one segment when its plan fits the budget, else the balanced K
static LongPlan long_plan(int32_t T, int32_t L, int64_t budget, int32_t segment_frames) {
  if (T <= 0) return LongPlan();
  if (segment_frames > 0) return long_plan_of(T, L, std::min<int64_t>(segment_frames, T));
  const LongPlan whole = long_plan_of(T, L, T);
  return whole.bytes <= budget ? whole : long_plan_of(T, L, long_balanced_frames(T));
}

#ifdef CTC_SIM
namespace {
struct AlignSeqCtx {
  enum { GROUPS = FORWARD_MAX_GROUPS };  // (ctc_forward_hyp: the one thread owns every group)
  int tid = 0, nt = 1;
  void sync() {}
};
}  // namespace
#endif

// ---- what the transcript calls share ---------------------------------------------------------------------------------------
// A call's constants: the alphabet's size, its blank and ln(MIN_TOKEN_CLIP_P) (constants.py:17)
struct TranscriptCall {
  int V = 0, blank = -1;
  double clip_lo = 0;
};

// What every entry point checks first, in this order: the pointers and counts it reads (args_ok, the decoder among them),
// the dtype, its own option (bad_option: the message, empty for a good one), the alphabet's blank.
static int transcript_open(const ctcdec_decoder* dec, bool args_ok, int32_t dtype, const std::string& bad_option, TranscriptCall& tc) {
  if (!args_ok) return fail(CTCDEC_ERR_ARG, "bad arguments");
  if (dtype < CTCDEC_F32 || dtype > CTCDEC_BF16) return fail(CTCDEC_ERR_ARG, "dtype must be f32, f64, f16 or bf16");
  if (!bad_option.empty()) return fail(CTCDEC_ERR_ARG, bad_option);
  tc.V = (int)dec->alpha.labels.size();
  for (int v = 0; v < tc.V && tc.blank < 0; ++v)
    if (dec->alpha.labels[(size_t)v].empty()) tc.blank = v;
  if (tc.blank < 0) return fail(CTCDEC_ERR_ARG, "the alphabet has no blank label");
  tc.clip_lo = log(1e-15);
  return CTCDEC_OK;
}
static std::string bad_fold(int32_t fold) {
  return fold != 0 && fold != LOGP_MEAN && fold != LOGP_MIN && fold != LOGP_MAX ? "unknown confidence fold" : "";
}
static std::string bad_kernel(int32_t kernel) {
  return kernel < 0 || kernel > 2 ? "kernel must be 0 (the library chooses), 1 (wave) or 2 (group)" : "";
}

// Where each utterance's rows start among the rows of the call: [n + 1]
static std::vector<int64_t> row_starts(const int32_t* frames, size_t n) {
  std::vector<int64_t> row0(n + 1, 0);
  for (size_t u = 0; u < n; ++u) row0[u + 1] = row0[u] + frames[u];
  return row0;
}

// The launches of a call: items in input order until their tables fill the budget. An item without a table (bytes_of(i) == 0:
// no frames, or nothing to launch) is in none of them. Returns the bytes of the largest launch's tables.
template <class BytesOf>
static int64_t budget_groups(int32_t n, BytesOf bytes_of, int64_t budget, std::vector<std::vector<int32_t>>& groups) {
  int64_t used = 0, most = 0;
  for (int32_t i = 0; i < n; ++i) {
    const int64_t bytes = bytes_of(i);
    if (bytes == 0) continue;
    if (groups.empty() || used + bytes > budget) {
      groups.emplace_back();
      used = 0;
    }
    groups.back().push_back(i);
    used += bytes;
    most = std::max(most, used);
  }
  return most;
}

// The labels of one target, who() in a message (formed only for one): inside the alphabet and not the blank, which the message
// calls `noun` and `not_a`. Returns through `need` the labels plus the adjacent equal labels: the fewest frames a path takes.
template <class Who>
static int check_labels(const int32_t* lab, int64_t L, int V, int blank, Who who, const char* noun, const char* not_a, int64_t& need) {
  need = L;
  for (int64_t k = 0; k < L; ++k) {
    const int32_t id = lab[k];
    if (id < 0 || id >= V) return fail(CTCDEC_ERR_ARG, who() + ": " + noun + " " + std::to_string(id) + " is outside the alphabet");
    if (id == blank) return fail(CTCDEC_ERR_ARG, who() + ": the blank is not a " + not_a);
    if (k > 0 && id == lab[k - 1]) ++need;
  }
  return CTCDEC_OK;
}

// Utterance u's frame count and matrix, for the calls that check nothing else about an utterance
static int check_frames(const void* const* utt_logits, const int32_t* utt_frames, int32_t u) {
  if (utt_frames[u] < 0) return fail(CTCDEC_ERR_ARG, "utterance " + std::to_string(u) + ": negative frame count");
  if (utt_frames[u] > 0 && !utt_logits[u]) return fail(CTCDEC_ERR_ARG, "utterance " + std::to_string(u) + ": no logits");
  return CTCDEC_OK;
}

// Everything the kernels index with comes from the caller: checked here, before anything moves.
static int check_alignment(const void* const* utt_logits, const int32_t* utt_frames, int32_t n_utts, const int32_t* targets,
                           const int64_t* target_off, int64_t budget, const TranscriptCall& tc, int32_t max_labels = ALIGN_MAX_LABELS,
                           int32_t segment_frames = -1) {
  const bool planned = segment_frames >= 0;  // ctcdec_align_long_batch: the budget bounds an utterance's plan, not its whole table
  if (target_off[0] != 0) return fail(CTCDEC_ERR_ARG, "target_off must start at 0");
  std::string infeasible;
  for (int32_t u = 0; u < n_utts; ++u) {
    const int64_t T = utt_frames[u], L = target_off[u + 1] - target_off[u];
    if (T < 0) return fail(CTCDEC_ERR_ARG, "negative frame count");
    if (L < 0) return fail(CTCDEC_ERR_ARG, "target_off must not decrease");
    if (L > max_labels)
      return fail(CTCDEC_ERR_LIMIT, "utterance " + std::to_string(u) + ": " + std::to_string(L) + " target labels, above the limit of " +
                                        std::to_string(max_labels) +
                                        (planned ? " (2L + 1 states below 2^21)" : " (two fp64 score columns of 2L + 1 states in LDS)"));
    if (L > 0 && !targets) return fail(CTCDEC_ERR_ARG, "no targets");
    if (T > 0 && !utt_logits[u]) return fail(CTCDEC_ERR_ARG, "utterance " + std::to_string(u) + ": no logits");
    int64_t need = 0;
    if (int rc = check_labels(targets + target_off[u], L, tc.V, tc.blank, [&] { return "utterance " + std::to_string(u); }, "target label",
                              "target label", need))
      return rc;
    if (T < need) infeasible += (infeasible.empty() ? "" : ", ") + std::to_string(u);
    if (planned) {
      const int64_t bytes = long_plan((int32_t)T, (int32_t)L, budget, segment_frames).bytes;
      if (bytes > budget)
        return fail(CTCDEC_ERR_LIMIT, "utterance " + std::to_string(u) + ": segment tables, checkpoints and columns of " + std::to_string(bytes) +
                                          " bytes, above the budget of " + std::to_string(budget) + " bytes for one launch");
    } else if (T * (int64_t)align_chunks((int32_t)L) > budget)
      return fail(CTCDEC_ERR_LIMIT, "utterance " + std::to_string(u) + ": a back-pointer table of " +
                                        std::to_string(T * (int64_t)align_chunks((int32_t)L)) + " bytes, above the budget of " +
                                        std::to_string(budget) + " bytes for one launch");
  }
  if (!infeasible.empty())
    return fail(CTCDEC_ERR_ARG, "no alignment path (fewer frames than target labels plus adjacent repeats) for utterances: " + infeasible);
  return CTCDEC_OK;
}

// What every transcript call does before its own recursion: the device lock taken (held while the AlignFront lives) and the
// device bound to the thread, host matrices staged (consecutive ones in one copy; device pointers are used in place),
// pointers and row offsets uploaded -- align_stage, all that a greedy decode without confidences needs --, the utterances
// classified as probabilities or logits, and row_lse over the rows of the logit utterances -- once per utterance.
struct AlignFront {
  std::unique_lock<std::mutex> device_lock;
  std::vector<const void*> ptrs;   // [n] device pointers of the utterances' matrices
  std::vector<uint32_t> is_prob;   // [n] the classification read back
  double* lse = nullptr;           // [R] (device) row log-sum-exps, indexed like row0
  double sniff_ms = 0;             // the classification's kernel time
  bool want_max = false;           // in: row_lse_max instead of row_lse (ctcdec_align_gaps_batch)
  double* rmax = nullptr;          // [R] (device, want_max) every row's largest entry that is not a NaN
  int want_arg_blank = -1;         // in: >= 0 (with want_max): row_lse_argmax, this the blank's index (ctcdec_greedy_batch)
  int32_t* arg = nullptr;          // [R] (device, want_arg_blank >= 0) every row's most probable label
};
static int align_stage(ctcdec_decoder* dec, const void* const* utt_logits, const int32_t* utt_frames, int32_t n_utts, int32_t dtype,
                       int32_t is_device, int V, const std::vector<int64_t>& row0, AlignFront& f) {
  std::string err;
  f.device_lock = std::unique_lock<std::mutex>(g_device_mu);
  if (be::bind_thread(&err)) return fail(CTCDEC_ERR_DEVICE, err);
  const size_t n = (size_t)n_utts;
  const int64_t R = row0[n];
  const size_t row_bytes = (size_t)V * dtype_size(dtype);
  std::vector<const void*>& ptrs = f.ptrs;
  ptrs.assign(n, nullptr);
  if (is_device) {
    for (size_t u = 0; u < n; ++u) ptrs[u] = utt_logits[u];
  } else {
    if (dec->w_logits.ensure((size_t)R * row_bytes, &err)) return fail(CTCDEC_ERR_DEVICE, err);
    for (size_t u = 0; u < n;) {
      char* dst = (char*)dec->w_logits.p + (size_t)row0[u] * row_bytes;
      const char* src = (const char*)utt_logits[u];
      size_t bytes = (size_t)utt_frames[u] * row_bytes;
      ptrs[u] = dst;
      size_t v = u + 1;
      while (v < n && (const char*)utt_logits[v] == src + bytes) {
        ptrs[v] = dst + bytes;
        bytes += (size_t)utt_frames[v] * row_bytes;
        ++v;
      }
      if (bytes && be::h2d(dst, src, bytes, &err)) return fail(CTCDEC_ERR_DEVICE, err);
      u = v;
    }
  }
  if (upload(dec->w_ptrs, ptrs, &err) || upload(dec->w_row0, row0, &err)) return fail(CTCDEC_ERR_DEVICE, err);
  return CTCDEC_OK;
}
// The front of a call that stages nothing: the device lock taken and the device bound, the kernels' timers reset
static int device_only_front(AlignFront& f) {
  std::string err;
  f.device_lock = std::unique_lock<std::mutex>(g_device_mu);
  if (be::bind_thread(&err)) return fail(CTCDEC_ERR_DEVICE, err);
#ifndef CTC_SIM
  be::align_timing_reset();
#endif
  return CTCDEC_OK;
}
// The one pass over the staged rows, by what the front has room for: f.lse alone (row_lse, over the rows of the logit
// utterances), with f.rmax (row_lse_max, every row), with f.arg too (row_lse_argmax), or f.arg alone (row_argmax: no
// classification is read). f.want_arg_blank: the blank's index for the last two. Resets the kernels' timers.
static int row_pass(ctcdec_decoder* dec, const int32_t* utt_frames, int32_t n_utts, int32_t dtype, int V, const std::vector<int64_t>& row0,
                    const AlignFront& f) {
#ifdef CTC_SIM  // (the simulator's device memory is host memory: the kernels' bodies, row by row and utterance by utterance)
  for (size_t u = 0; u < (size_t)n_utts; ++u)
    for (int64_t t = 0; t < utt_frames[u]; ++t) {
      const int64_t r = row0[u] + t;
      const size_t at = (size_t)t * (size_t)V;
      if (f.rmax) row_lse_max_seq(f.ptrs[u], dtype, at, V, f.is_prob[u] != 0, &f.lse[r], &f.rmax[r]);
      else if (f.lse && !f.is_prob[u]) f.lse[r] = row_lse_seq(f.ptrs[u], dtype, at, V);
      if (f.arg) f.arg[r] = row_argmax_seq(f.ptrs[u], dtype, at, V, f.want_arg_blank);
    }
#else
  std::string err;
  be::align_timing_reset();
  be::RowLseArgs la;
  la.utt_logits = (const void* const*)dec->w_ptrs.p;
  la.utt_row0 = (const int64_t*)dec->w_row0.p;
  la.utt_is_prob = f.lse ? (const uint32_t*)dec->w_isprob.p : nullptr;
  la.n_utts = n_utts;
  la.n_rows = row0[(size_t)n_utts];
  la.n_labels = V;
  la.dtype = dtype;
  la.lse = f.lse;
  if (!f.lse ? be::launch_row_argmax(la, f.arg, f.want_arg_blank, &err)
      : f.arg ? be::launch_row_lse_argmax(la, f.rmax, f.arg, f.want_arg_blank, &err)
      : f.rmax ? be::launch_row_lse_max(la, f.rmax, &err) : be::launch_row_lse(la, &err))
    return fail(CTCDEC_ERR_DEVICE, err);
#endif
  return CTCDEC_OK;
}
static int align_front(ctcdec_decoder* dec, const void* const* utt_logits, const int32_t* utt_frames, int32_t n_utts, int32_t dtype,
                       int32_t is_device, int V, const std::vector<int64_t>& row0, AlignFront& f) {
  if (int rc = align_stage(dec, utt_logits, utt_frames, n_utts, dtype, is_device, V, row0, f)) return rc;
  std::string err;
  const size_t n = (size_t)n_utts;
  const int64_t R = row0[n];
  std::vector<const void*>& ptrs = f.ptrs;
  // probabilities or logits? The decode's own prune stage decides (pass 0 and its sniff, the exact test for the ambiguous),
  // at a threshold nothing but a certain label passes: its survivor lists are three entries wide and are not looked at.
  PruneStage s{dec, &ptrs, n_utts, dtype, R, V, 0.0};
  if (int rc = prune_stage(s, nullptr)) return rc;
  f.is_prob.assign(n, 0);
  if (be::d2h(f.is_prob.data(), dec->w_isprob.p, n * 4, &err)) return fail(CTCDEC_ERR_DEVICE, err);
  double beam_ms = 0;
  be::last_timing(&f.sniff_ms, &beam_ms);
  if (dec->w_alse.ensure((size_t)R * 8, &err)) return fail(CTCDEC_ERR_DEVICE, err);
  f.lse = (double*)dec->w_alse.p;
  if (f.want_max) {
    if (dec->w_amax.ensure((size_t)R * 8, &err)) return fail(CTCDEC_ERR_DEVICE, err);
    f.rmax = (double*)dec->w_amax.p;
  }
  if (f.want_max && f.want_arg_blank >= 0) {
    if (dec->w_garg.ensure((size_t)R * 4, &err)) return fail(CTCDEC_ERR_DEVICE, err);
    f.arg = (int32_t*)dec->w_garg.p;
  }
  return row_pass(dec, utt_frames, n_utts, dtype, V, row0, f);
}

// What ctcdec_align_gaps_batch adds to a Viterbi call: one flag per slot of every utterance (L + 1 of them from off[u]) and,
// out, the sum of g(t) over each gap slot's frames
struct GapSlots {
  std::vector<uint8_t> gap;
  std::vector<int64_t> off;
  std::vector<double> logp;
};

// The call behind ctcdec_align_batch (Utt = AlignUtt, no slots), ctcdec_align_gaps_batch (Utt = GapsUtt) and
// ctcdec_align_long_batch (Utt = AlignLongUtt, with every utterance's plan): the checked labels of every utterance to a
// result with its paths, spans, scores and, with a fold, confidences.
template <class Utt>
static int viterbi_call(ctcdec_decoder* dec, const TranscriptCall& tc, const void* const* utt_logits, const int32_t* utt_frames,
                        int32_t n_utts, int32_t dtype, int32_t is_device, const int32_t* labels, const int64_t* lab_off, int32_t fold,
                        int64_t budget, GapSlots* slots, const std::vector<LongPlan>* plans, std::unique_ptr<ctcdec_alignment>& res) {
  constexpr bool GAPS = std::is_same<Utt, GapsUtt>::value, LONG = std::is_same<Utt, AlignLongUtt>::value;
  res.reset(new ctcdec_alignment());
  const size_t n = (size_t)n_utts;
  for (size_t u = 0; u < n; ++u) {
    res->seg_frames.push_back(LONG ? (*plans)[u].K : utt_frames[u]);
    res->n_segs.push_back(LONG ? (*plans)[u].n_seg : 1);
  }
  const int64_t NL = lab_off[n], NS = GAPS ? slots->off[n] : 0;
  const std::vector<int64_t> row0 = row_starts(utt_frames, n);
  const int64_t R = row0[n];
  res->has_gaps = GAPS;
  res->path_off = row0;
  res->tok_off.assign(lab_off, lab_off + n + 1);
  res->label.assign(labels, labels + NL);
  res->path.resize((size_t)R);
  res->start.assign((size_t)NL, 0);
  res->end.assign((size_t)NL, 0);
  res->score.assign(n, 0.0);
  res->has_logp = fold != 0;
  if (fold) res->logp.assign((size_t)NL, 0.0);
  if (GAPS) slots->logp.assign((size_t)NS, 0.0);
  if (R == 0) return CTCDEC_OK;
  std::string err;
  AlignFront fr;
  fr.want_max = GAPS;
  if (int rc = align_front(dec, utt_logits, utt_frames, n_utts, dtype, is_device, tc.V, row0, fr)) return rc;
  res->ms[0] = fr.sniff_ms;
  const size_t nl1 = (size_t)std::max<int64_t>(NL, 1);
  if (dec->w_apath.ensure((size_t)R * 4, &err) || dec->w_alab.ensure(nl1 * 4, &err) || dec->w_atok.ensure(nl1 * 8, &err) ||
      dec->w_atlp.ensure(nl1 * 8, &err) || dec->w_ascore.ensure(n * 8, &err) ||
      (GAPS && (dec->w_agap.ensure((size_t)NS, &err) || dec->w_aglp.ensure((size_t)NS * 8, &err))))
    return fail(CTCDEC_ERR_DEVICE, err);
  if ((NL && be::h2d(dec->w_alab.p, labels, (size_t)NL * 4, &err)) || be::zero(dec->w_atok.p, nl1 * 8, &err) ||
      be::zero(dec->w_atlp.p, nl1 * 8, &err) || be::zero(dec->w_ascore.p, n * 8, &err) ||
      (GAPS && (be::h2d(dec->w_agap.p, slots->gap.data(), (size_t)NS, &err) || be::zero(dec->w_aglp.p, (size_t)NS * 8, &err))))
    return fail(CTCDEC_ERR_DEVICE, err);
  // launches: utterances in input order until their back-pointer tables (LONG: their planned bytes) fill the budget; longest
  // first inside a launch
  const auto chunks_of = [&](int32_t u) { return align_chunks((int32_t)(lab_off[u + 1] - lab_off[u])); };
  // (LONG) the bytes of an utterance's segment table, and the doubles of its two columns and its checkpoints: the plan's terms
  const auto table_of = [&](int32_t u) { return LONG ? (int64_t)(*plans)[(size_t)u].K * chunks_of(u) : (int64_t)utt_frames[u] * chunks_of(u); };
  const auto doubles_of = [&](int32_t u) { return LONG ? ((*plans)[(size_t)u].bytes - table_of(u)) / 8 : (int64_t)0; };
  std::vector<std::vector<int32_t>> groups;
  int64_t most = budget_groups(n_utts, [&](int32_t u) { return LONG ? (*plans)[(size_t)u].bytes : table_of(u); }, budget, groups);
  if constexpr (LONG) {  // the two workspaces of a launch, each by the launch that needs most of it
    int64_t most_doubles = 0;
    most = 0;
    for (const auto& g : groups) {
      int64_t tables = 0, doubles = 0;
      for (int32_t u : g) tables += table_of(u), doubles += doubles_of(u);
      most = std::max(most, tables), most_doubles = std::max(most_doubles, doubles);
    }
    if (dec->w_lcol.ensure((size_t)std::max<int64_t>(most_doubles, 1) * 8, &err)) return fail(CTCDEC_ERR_DEVICE, err);
  }
  if (dec->w_abp.ensure((size_t)std::max<int64_t>(most, 1), &err)) return fail(CTCDEC_ERR_DEVICE, err);
  std::vector<Utt> utts;
  for (auto& g : groups) {
    std::stable_sort(g.begin(), g.end(), [&](int32_t a, int32_t b) { return utt_frames[a] > utt_frames[b]; });
    utts.clear();
    int64_t bp_off = 0, col_off = 0;
    int32_t max_chunks = 1;
    for (int32_t u : g) {
      const int64_t lo = lab_off[u];
      Utt a;
      a.x = fr.ptrs[(size_t)u];
      a.lse = fr.lse + row0[(size_t)u];
      a.lab = (const int32_t*)dec->w_alab.p + lo;
      a.bp = (uint8_t*)dec->w_abp.p + bp_off;
      a.path = (int32_t*)dec->w_apath.p + row0[(size_t)u];
      a.tok_start = (int32_t*)dec->w_atok.p + lo;
      a.tok_end = (int32_t*)dec->w_atok.p + NL + lo;
      a.tok_logp = (double*)dec->w_atlp.p + lo;
      a.score = (double*)dec->w_ascore.p + u;
      a.T = utt_frames[u];
      a.L = (int32_t)(lab_off[u + 1] - lo);
      a.is_prob = fr.is_prob[(size_t)u] ? 1 : 0;
      if constexpr (LONG) {
        a.K = (*plans)[(size_t)u].K;
        a.col = (double*)dec->w_lcol.p + col_off;
        a.ckpt = a.col + 8 * (int64_t)chunks_of(u);  // (read only when there is more than one segment)
        col_off += doubles_of(u);
      } else {
        a.pad = 0;
      }
      if constexpr (GAPS) {
        a.rmax = fr.rmax + row0[(size_t)u];
        a.gap = (const uint8_t*)dec->w_agap.p + slots->off[(size_t)u];
        a.gap_logp = (double*)dec->w_aglp.p + slots->off[(size_t)u];
      }
      utts.push_back(a);
      bp_off += table_of(u);
      max_chunks = std::max(max_chunks, chunks_of(u));
    }
#ifdef CTC_SIM
    std::vector<double> col((size_t)(GAPS ? 2 : LONG ? 0 : 8) * (size_t)max_chunks);  // (LONG: the columns are the record's)
    AlignSeqCtx cx;
    for (const Utt& a : utts) {
      if constexpr (GAPS)
        for_dtype(dtype, [&](auto dt) { ctc_viterbi_gaps_utt<decltype(dt)::value>(cx, a, tc.V, tc.blank, fold, tc.clip_lo, col.data()); });
      else if constexpr (LONG)
        ctc_viterbi_long_utt(cx, a, tc.V, dtype, tc.blank, fold, tc.clip_lo);
      else
        ctc_viterbi_utt(cx, a, tc.V, dtype, tc.blank, fold, tc.clip_lo, col.data());
    }
#else
    DevBuf& records = GAPS ? dec->w_agutts : LONG ? dec->w_lutts : dec->w_autts;
    if (upload(records, utts, &err)) return fail(CTCDEC_ERR_DEVICE, err);
    typename std::conditional<GAPS, be::ViterbiGapsArgs, typename std::conditional<LONG, be::ViterbiLongArgs, be::ViterbiArgs>::type>::type va;
    va.utts = (const Utt*)records.p;
    va.n_utts = (int32_t)utts.size();
    va.n_labels = tc.V;
    va.dtype = dtype;
    va.blank = tc.blank;
    va.fold = fold;
    if constexpr (LONG) va.pad = 0;
    else va.max_chunks = max_chunks;
    va.clip_lo = tc.clip_lo;
    int rc;
    if constexpr (GAPS) rc = be::launch_ctc_viterbi_gaps(va, &err);
    else if constexpr (LONG) rc = be::launch_ctc_viterbi_long(va, &err);
    else rc = be::launch_ctc_viterbi(va, &err);
    if (rc) return fail(CTCDEC_ERR_DEVICE, err);
#endif
    ++res->launches;
  }
  if (be::d2h(res->path.data(), dec->w_apath.p, (size_t)R * 4, &err) || be::d2h(res->score.data(), dec->w_ascore.p, n * 8, &err))
    return fail(CTCDEC_ERR_DEVICE, err);
  if (NL && (be::d2h(res->start.data(), dec->w_atok.p, (size_t)NL * 4, &err) ||
             be::d2h(res->end.data(), (const int32_t*)dec->w_atok.p + NL, (size_t)NL * 4, &err) ||
             (fold && be::d2h(res->logp.data(), dec->w_atlp.p, (size_t)NL * 8, &err))))
    return fail(CTCDEC_ERR_DEVICE, err);
  if (GAPS && be::d2h(slots->logp.data(), dec->w_aglp.p, (size_t)NS * 8, &err)) return fail(CTCDEC_ERR_DEVICE, err);
#ifndef CTC_SIM
  res->ms[1] = be::align_kernel_ms(GAPS ? be::K_ROW_LSE_MAX : be::K_ROW_LSE);
  res->ms[2] = be::align_kernel_ms(GAPS ? be::K_VITERBI_GAPS : LONG ? be::K_VITERBI_LONG : be::K_VITERBI);
#endif
  return CTCDEC_OK;
}

extern "C" {

int ctcdec_align_batch(ctcdec_decoder* dec, const void* const* utt_logits, const int32_t* utt_frames, int32_t n_utts, int32_t dtype,
                       int32_t is_device, const int32_t* targets, const int64_t* target_off, int32_t fold, int64_t bp_budget,
                       ctcdec_alignment** out) {
  TranscriptCall tc;
  const bool args_ok = dec && out && n_utts >= 0 && target_off && bp_budget >= 0 && (n_utts == 0 || (utt_logits && utt_frames));
  if (int rc = transcript_open(dec, args_ok, dtype, bad_fold(fold), tc)) return rc;
  const int64_t budget = bp_budget ? bp_budget : ALIGN_BP_BUDGET;
  if (int rc = check_alignment(utt_logits, utt_frames, n_utts, targets, target_off, budget, tc)) return rc;
  const auto t_begin = Clock::now();
  std::unique_ptr<ctcdec_alignment> res;
  if (int rc = viterbi_call<AlignUtt>(dec, tc, utt_logits, utt_frames, n_utts, dtype, is_device, targets, target_off, fold, budget,
                                      nullptr, nullptr, res))
    return rc;
  res->ms[3] = ms(t_begin, Clock::now());
  *out = res.release();
  return CTCDEC_OK;
}

int ctcdec_alignment_paths(const ctcdec_alignment* a, const int64_t** path_off_out, const int32_t** path_out, const double** score_out,
                           int64_t* n_utts_out) {
  if (!a || !path_off_out || !path_out || !score_out || !n_utts_out) return fail(CTCDEC_ERR_ARG, "no alignment");
  *path_off_out = a->path_off.data();
  *path_out = a->path.data();
  *score_out = a->score.data();
  *n_utts_out = (int64_t)a->score.size();
  return CTCDEC_OK;
}

int ctcdec_alignment_tokens(const ctcdec_alignment* a, const int64_t** tok_off_out, const int32_t** label_out, const int32_t** start_out,
                            const int32_t** end_out, const double** logp_out, int64_t* n_tokens_out) {
  if (!a || !tok_off_out || !label_out || !start_out || !end_out || !logp_out || !n_tokens_out) return fail(CTCDEC_ERR_ARG, "no alignment");
  *tok_off_out = a->tok_off.data();
  *label_out = a->label.data();
  *start_out = a->start.data();
  *end_out = a->end.data();
  *logp_out = a->has_logp ? a->logp.data() : nullptr;
  *n_tokens_out = (int64_t)a->label.size();
  return CTCDEC_OK;
}

int ctcdec_alignment_timing(const ctcdec_alignment* a, double* ms4, int32_t* launches_out) {
  if (!a || !ms4) return fail(CTCDEC_ERR_ARG, "no alignment");
  for (int k = 0; k < 4; ++k) ms4[k] = a->ms[k];
  if (launches_out) *launches_out = a->launches;
  return CTCDEC_OK;
}

void ctcdec_alignment_free(ctcdec_alignment* a) { delete a; }

// ---- forced alignment of long transcripts ("Forced alignment of long transcripts") -----------------------------
int ctcdec_align_long_batch(ctcdec_decoder* dec, const void* const* utt_logits, const int32_t* utt_frames, int32_t n_utts, int32_t dtype,
                            int32_t is_device, const int32_t* targets, const int64_t* target_off, int32_t fold, int64_t bp_budget,
                            int32_t segment_frames, ctcdec_alignment** out) {
  TranscriptCall tc;
  const bool args_ok = dec && out && n_utts >= 0 && target_off && bp_budget >= 0 && (n_utts == 0 || (utt_logits && utt_frames));
  const std::string bad_option = !bad_fold(fold).empty() ? bad_fold(fold) : segment_frames < 0 ? "segment_frames must not be negative" : "";
  if (int rc = transcript_open(dec, args_ok, dtype, bad_option, tc)) return rc;
  const int64_t budget = bp_budget ? bp_budget : ALIGN_BP_BUDGET;
  if (int rc = check_alignment(utt_logits, utt_frames, n_utts, targets, target_off, budget, tc, ALIGN_LONG_MAX_LABELS, segment_frames))
    return rc;
  std::vector<LongPlan> plans;
  for (int32_t u = 0; u < n_utts; ++u)
    plans.push_back(long_plan(utt_frames[u], (int32_t)(target_off[u + 1] - target_off[u]), budget, segment_frames));
  const auto t_begin = Clock::now();
  std::unique_ptr<ctcdec_alignment> res;
  if (int rc = viterbi_call<AlignLongUtt>(dec, tc, utt_logits, utt_frames, n_utts, dtype, is_device, targets, target_off, fold, budget,
                                          nullptr, &plans, res))
    return rc;
  res->ms[3] = ms(t_begin, Clock::now());
  *out = res.release();
  return CTCDEC_OK;
}

int ctcdec_alignment_plan(const ctcdec_alignment* a, const int32_t** segment_frames_out, const int32_t** n_segments_out,
                          int64_t* n_utts_out) {
  if (!a || !segment_frames_out || !n_segments_out || !n_utts_out) return fail(CTCDEC_ERR_ARG, "no alignment");
  *segment_frames_out = a->seg_frames.data();
  *n_segments_out = a->n_segs.data();
  *n_utts_out = (int64_t)a->seg_frames.size();
  return CTCDEC_OK;
}

// ---- alignment with gaps ("Alignment with gaps") -------------------------------------------------------------
int ctcdec_align_gaps_batch(ctcdec_decoder* dec, const void* const* utt_logits, const int32_t* utt_frames, int32_t n_utts, int32_t dtype,
                            int32_t is_device, const int32_t* targets, const int64_t* target_off, int32_t fold, int64_t bp_budget,
                            ctcdec_alignment** out) {
  TranscriptCall tc;
  const bool args_ok = dec && out && n_utts >= 0 && target_off && bp_budget >= 0 && (n_utts == 0 || (utt_logits && utt_frames));
  if (int rc = transcript_open(dec, args_ok, dtype, bad_fold(fold), tc)) return rc;
  const int64_t budget = bp_budget ? bp_budget : ALIGN_BP_BUDGET;
  const size_t n = (size_t)n_utts;
  // the items apart: the labels, with offsets of their own, and one flag per slot (before label 0, between neighbours, after
  // the last label). Everything align checks is then checked by align's own code, on the labels.
  if (target_off[0] != 0) return fail(CTCDEC_ERR_ARG, "target_off must start at 0");
  std::vector<int32_t> labels;
  std::vector<int64_t> lab_off(n + 1, 0);
  GapSlots slots;
  slots.off.assign(n + 1, 0);
  for (size_t u = 0; u < n; ++u) {
    const int64_t N = target_off[u + 1] - target_off[u];
    if (N < 0) return fail(CTCDEC_ERR_ARG, "target_off must not decrease");
    if (N > 0 && !targets) return fail(CTCDEC_ERR_ARG, "no targets");
    slots.gap.push_back(0);
    for (int64_t k = 0; k < N; ++k) {
      const int32_t id = targets[target_off[u] + k];
      if (id != CTCDEC_ALIGN_GAP) {
        labels.push_back(id);
        slots.gap.push_back(0);
        continue;
      }
      if (k > 0 && targets[target_off[u] + k - 1] == CTCDEC_ALIGN_GAP)
        return fail(CTCDEC_ERR_ARG, "utterance " + std::to_string(u) + ": two adjacent gaps are one gap");
      slots.gap.back() = 1;
    }
    lab_off[u + 1] = (int64_t)labels.size();
    slots.off[u + 1] = (int64_t)slots.gap.size();
  }
  if (labels.empty()) labels.push_back(0);  // (never read: .data() of an empty vector may be null)
  if (int rc = check_alignment(utt_logits, utt_frames, n_utts, labels.data(), lab_off.data(), budget, tc)) return rc;
  for (size_t u = 0; u < n; ++u)
    if (lab_off[u + 1] == lab_off[u])
      return fail(CTCDEC_ERR_ARG, "utterance " + std::to_string(u) + ": a target needs at least one label");
  const auto t_begin = Clock::now();
  std::unique_ptr<ctcdec_alignment> res;
  if (int rc = viterbi_call<GapsUtt>(dec, tc, utt_logits, utt_frames, n_utts, dtype, is_device, labels.data(), lab_off.data(), fold,
                                     budget, &slots, nullptr, res))
    return rc;
  // the gaps, in target order: everything between the end of the label before and the start of the label after
  res->gap_off.assign(n + 1, 0);
  for (size_t u = 0; u < n; ++u) {
    const int64_t lo = lab_off[u], L = lab_off[u + 1] - lo;
    for (int64_t j = 0; j <= L; ++j) {
      if (!slots.gap[(size_t)(slots.off[u] + j)]) continue;
      res->gap_start.push_back(j > 0 ? res->end[(size_t)(lo + j - 1)] : 0);
      res->gap_end.push_back(j < L ? res->start[(size_t)(lo + j)] : utt_frames[u]);
      res->gap_logp.push_back(slots.logp[(size_t)(slots.off[u] + j)]);
    }
    res->gap_off[u + 1] = (int64_t)res->gap_start.size();
  }
  res->ms[3] = ms(t_begin, Clock::now());
  *out = res.release();
  return CTCDEC_OK;
}

int ctcdec_alignment_gaps(const ctcdec_alignment* a, const int64_t** gap_off_out, const int32_t** start_out, const int32_t** end_out,
                          const double** logp_out, int64_t* n_gaps_out) {
  if (!a || !gap_off_out || !start_out || !end_out || !logp_out || !n_gaps_out) return fail(CTCDEC_ERR_ARG, "no alignment");
  if (!a->has_gaps) return fail(CTCDEC_ERR_ARG, "the alignment was made without gaps (ctcdec_align_batch)");
  *gap_off_out = a->gap_off.data();
  *start_out = a->gap_start.data();
  *end_out = a->gap_end.data();
  *logp_out = a->gap_logp.data();
  *n_gaps_out = (int64_t)a->gap_start.size();
  return CTCDEC_OK;
}

// ---- transcript likelihood ("Transcript likelihood") -----------------------------------------------------------
}  // extern "C"

// ---- greedy decode ("Greedy decode") ---------------------------------------------------------------------------------
struct ctcdec_greedy {
  std::vector<int64_t> tok_off, text_off;
  std::vector<int32_t> label, start, end;
  std::vector<double> logp, score;
  std::string texts;
  bool has_fold = false;
  int32_t launches = 0;
  double ms[4] = {0, 0, 0, 0};
  double lse_ms = 0;
};

#ifdef CTC_SIM
namespace {
struct GreedySeqCtx {  // (greedy_collapse_utt: a "wave" of one lane, a frame a step)
  int lane() const { return 0; }
  int lanes() const { return 1; }
  int32_t up(int32_t v) const { return v; }
  int32_t down(int32_t v) const { return v; }
  int32_t first(int32_t v) const { return v; }
  int32_t last(int32_t v) const { return v; }
  uint64_t ballot(bool b) const { return b ? 1u : 0u; }
  void publish() const {}
};
}  // namespace
#endif

// The text of a sequence of token labels, as decoder.py's _words_of_target forms it: under a character alphabet the space label
// ends a word and the other labels are its pieces; under a BPE alphabet a label that begins with the mark, or follows one
// that ends with it (and is more than the mark alone), begins a word, and the pieces are the labels without the marks at
// either end. Words are joined by one space; a word of empty pieces alone (the bare mark) is a word too and takes its
// separator. What a label contributes is worked out once per call, not once per token.
struct GreedyWords {
  std::vector<std::string> piece;          // what the label appends to its word
  std::vector<uint8_t> ends, begins, forces;  // the space label; a leading mark; a trailing mark on more than the mark alone
  explicit GreedyWords(const HostAlphabet& alpha) {
    static const std::string MARK = "\xE2\x96\x81";  // U+2581
    const size_t V = alpha.labels.size(), m = MARK.size();
    piece.resize(V);
    ends.assign(V, 0), begins.assign(V, 0), forces.assign(V, 0);
    for (size_t c = 0; c < V; ++c) {
      const std::string& l = alpha.labels[c];
      if (!alpha.is_bpe) {
        ends[c] = l == " ";
        piece[c] = l;
        continue;
      }
      begins[c] = l.compare(0, m, MARK) == 0;
      forces[c] = utf8_length(l.data(), l.size()) > 1 && l.size() >= m && l.compare(l.size() - m, m, MARK) == 0;
      size_t a = 0, b = l.size();  // str.strip(mark): every mark at either end
      while (b - a >= m && l.compare(a, m, MARK) == 0) a += m;
      while (b - a >= m && l.compare(b - m, m, MARK) == 0) b -= m;
      piece[c] = l.substr(a, b - a);
    }
  }
  void append_text(const int32_t* lab, int64_t n, std::string& out) const {
    bool open = false, any_word = false, force = false;  // a word has a piece; the text has a word; the next label begins a word
    for (int64_t k = 0; k < n; ++k) {
      const size_t c = (size_t)lab[k];
      if (ends[c]) {
        open = false;
        continue;
      }
      if (force || begins[c]) open = false;
      force = forces[c] != 0;
      if (!open) {
        if (any_word) out += ' ';
        open = any_word = true;
      }
      out += piece[c];
    }
  }
};

static int greedy_call(ctcdec_decoder* dec, const TranscriptCall& tc, const void* const* utt_logits, const int32_t* utt_frames,
                       int32_t n_utts, int32_t dtype, int32_t is_device, int32_t fold, std::unique_ptr<ctcdec_greedy>& res) {
  res.reset(new ctcdec_greedy());
  const size_t n = (size_t)n_utts;
  const std::vector<int64_t> row0 = row_starts(utt_frames, n);
  const int64_t R = row0[n];
  res->has_fold = fold != 0;
  res->tok_off.assign(n + 1, 0);
  res->text_off.assign(n + 1, 0);
  if (fold) res->score.assign(n, 0.0);
  if (R == 0) return CTCDEC_OK;  // (no frames: no tokens, empty texts, nothing launched)
  std::string err;
  AlignFront fr;
  if (fold) {
    fr.want_max = true;
    fr.want_arg_blank = tc.blank;
    if (int rc = align_front(dec, utt_logits, utt_frames, n_utts, dtype, is_device, tc.V, row0, fr)) return rc;
    res->ms[0] = fr.sniff_ms;
  } else {
    // every logit is read once, by row_argmax: no classification, no log-sum-exp
    if (int rc = align_stage(dec, utt_logits, utt_frames, n_utts, dtype, is_device, tc.V, row0, fr)) return rc;
    if (dec->w_garg.ensure((size_t)R * 4, &err)) return fail(CTCDEC_ERR_DEVICE, err);
    fr.arg = (int32_t*)dec->w_garg.p;
    fr.want_arg_blank = tc.blank;
    if (int rc = row_pass(dec, utt_frames, n_utts, dtype, tc.V, row0, fr)) return rc;
  }
  ++res->launches;
  // the count pass, the host's scan of n counts, the write pass
  if (dec->w_gcnt.ensure(n * 4, &err)) return fail(CTCDEC_ERR_DEVICE, err);
  GreedyArgs ga;
  memset(&ga, 0, sizeof(ga));
  ga.arg = fr.arg;
  ga.row0 = (const int64_t*)dec->w_row0.p;
  ga.count = (int32_t*)dec->w_gcnt.p;
  ga.n_utts = n_utts;
  ga.blank = tc.blank;
  ga.fold = fold;
  ga.write = 0;
  ga.clip_lo = tc.clip_lo;
  const auto collapse = [&]() -> int {
#ifdef CTC_SIM
    GreedySeqCtx cx;
    for (int32_t u = 0; u < n_utts; ++u) greedy_collapse_utt(cx, ga, u);
#else
    if (be::launch_greedy_collapse(ga, &err)) return fail(CTCDEC_ERR_DEVICE, err);
#endif
    ++res->launches;
    return CTCDEC_OK;
  };
  if (int rc = collapse()) return rc;
  std::vector<int32_t> count(n, 0);
  if (be::d2h(count.data(), dec->w_gcnt.p, n * 4, &err)) return fail(CTCDEC_ERR_DEVICE, err);
  for (size_t u = 0; u < n; ++u) {
    if (count[u] < 0 || count[u] > utt_frames[u]) return fail(CTCDEC_ERR_INTERNAL, "greedy_collapse counted more tokens than frames");
    res->tok_off[u + 1] = res->tok_off[u] + count[u];
  }
  const int64_t NT = res->tok_off[n];
  const size_t nt1 = (size_t)std::max<int64_t>(NT, 1);
  if (upload(dec->w_gtoff, res->tok_off, &err) || dec->w_glab.ensure(nt1 * 4, &err) || dec->w_gspan.ensure(nt1 * 8, &err) ||
      (fold && (dec->w_glogp.ensure(nt1 * 8, &err) || dec->w_ascore.ensure(n * 8, &err))))
    return fail(CTCDEC_ERR_DEVICE, err);
  ga.write = 1;
  ga.tok_off = (const int64_t*)dec->w_gtoff.p;
  ga.label = (int32_t*)dec->w_glab.p;
  ga.start = (int32_t*)dec->w_gspan.p;
  ga.end = (int32_t*)dec->w_gspan.p + nt1;
  if (fold) {
    ga.lse = fr.lse;
    ga.rmax = fr.rmax;
    ga.is_prob = (const uint32_t*)dec->w_isprob.p;
    ga.logp = (double*)dec->w_glogp.p;
    ga.score = (double*)dec->w_ascore.p;
  }
  if (int rc = collapse()) return rc;
  // one copy per array, of the tokens' size
  res->label.resize((size_t)NT);
  res->start.resize((size_t)NT);
  res->end.resize((size_t)NT);
  if (fold) res->logp.resize((size_t)NT);
  if (NT && (be::d2h(res->label.data(), ga.label, (size_t)NT * 4, &err) || be::d2h(res->start.data(), ga.start, (size_t)NT * 4, &err) ||
             be::d2h(res->end.data(), ga.end, (size_t)NT * 4, &err) || (fold && be::d2h(res->logp.data(), ga.logp, (size_t)NT * 8, &err))))
    return fail(CTCDEC_ERR_DEVICE, err);
  if (fold && be::d2h(res->score.data(), ga.score, n * 8, &err)) return fail(CTCDEC_ERR_DEVICE, err);
#ifndef CTC_SIM
  res->ms[1] = be::align_kernel_ms(fold ? be::K_ROW_LSE_ARGMAX : be::K_ROW_ARGMAX);
  res->ms[2] = be::align_kernel_ms(be::K_GREEDY_COLLAPSE);
  res->lse_ms = fold ? res->ms[1] : 0.0;
  // (AlignFront::sniff_ms comes from be::last_timing, which reports nothing for a prune stage that no beam launch follows)
  if (fold) res->ms[0] = be::last_prune_ms();
#endif
  // the texts, on the host. No kernel formed an address from a label: they are checked here, before they index the alphabet.
  for (int64_t k = 0; k < NT; ++k)
    if (res->label[(size_t)k] < 0 || res->label[(size_t)k] >= tc.V || res->label[(size_t)k] == tc.blank)
      return fail(CTCDEC_ERR_INTERNAL, "greedy decode: a token's label is outside the alphabet");
  const GreedyWords words(dec->alpha);
  for (size_t u = 0; u < n; ++u) {
    words.append_text(res->label.data() + res->tok_off[u], res->tok_off[u + 1] - res->tok_off[u], res->texts);
    res->text_off[u + 1] = (int64_t)res->texts.size();
  }
  return CTCDEC_OK;
}

extern "C" {

int ctcdec_greedy_batch(ctcdec_decoder* dec, const void* const* utt_logits, const int32_t* utt_frames, int32_t n_utts, int32_t dtype,
                        int32_t is_device, int32_t fold, ctcdec_greedy** out) {
  TranscriptCall tc;
  const bool args_ok = dec && out && n_utts >= 0 && (n_utts == 0 || (utt_logits && utt_frames));
  if (int rc = transcript_open(dec, args_ok, dtype, bad_fold(fold), tc)) return rc;
  for (int32_t u = 0; u < n_utts; ++u)
    if (int rc = check_frames(utt_logits, utt_frames, u)) return rc;
  const auto t_begin = Clock::now();
  std::unique_ptr<ctcdec_greedy> res;
  if (int rc = greedy_call(dec, tc, utt_logits, utt_frames, n_utts, dtype, is_device, fold, res)) return rc;
  res->ms[3] = ms(t_begin, Clock::now());
  *out = res.release();
  return CTCDEC_OK;
}

int ctcdec_greedy_texts(const ctcdec_greedy* g, const char** blob_out, const int64_t** off_out, int64_t* n_utts_out) {
  if (!g || !blob_out || !off_out || !n_utts_out) return fail(CTCDEC_ERR_ARG, "no greedy result");
  *blob_out = g->texts.data();
  *off_out = g->text_off.data();
  *n_utts_out = (int64_t)g->text_off.size() - 1;
  return CTCDEC_OK;
}

int ctcdec_greedy_tokens(const ctcdec_greedy* g, const int64_t** tok_off_out, const int32_t** label_out, const int32_t** start_out,
                         const int32_t** end_out, const double** logp_out, int64_t* n_tokens_out) {
  if (!g || !tok_off_out || !label_out || !start_out || !end_out || !logp_out || !n_tokens_out) return fail(CTCDEC_ERR_ARG, "no greedy result");
  *tok_off_out = g->tok_off.data();
  *label_out = g->label.data();
  *start_out = g->start.data();
  *end_out = g->end.data();
  *logp_out = g->has_fold ? g->logp.data() : nullptr;
  *n_tokens_out = (int64_t)g->label.size();
  return CTCDEC_OK;
}

int ctcdec_greedy_scores(const ctcdec_greedy* g, const double** score_out, int64_t* n_utts_out) {
  if (!g || !score_out || !n_utts_out) return fail(CTCDEC_ERR_ARG, "no greedy result");
  *score_out = g->has_fold ? g->score.data() : nullptr;
  *n_utts_out = (int64_t)g->tok_off.size() - 1;
  return CTCDEC_OK;
}

int ctcdec_greedy_timing(const ctcdec_greedy* g, double* ms4, int32_t* launches_out, double* lse_ms_out) {
  if (!g || !ms4) return fail(CTCDEC_ERR_ARG, "no greedy result");
  for (int k = 0; k < 4; ++k) ms4[k] = g->ms[k];
  if (launches_out) *launches_out = g->launches;
  if (lse_ms_out) *lse_ms_out = g->lse_ms;
  return CTCDEC_OK;
}

void ctcdec_greedy_free(ctcdec_greedy* g) { delete g; }

}  // extern "C"

// Everything ctcdec_score_batch indexes with comes from the caller: checked here, in the order in which one array bounds the
// next, before anything moves. need[h]: labels plus adjacent equal labels of hypothesis h. (ctcdec_find_batch checks its
// phrases with it too: `item` is what a message calls an entry.)
static int check_scores(const void* const* utt_logits, const int32_t* utt_frames, int32_t n_utts, const int32_t* targets,
                        const int64_t* target_off, const int64_t* hyp_off, const TranscriptCall& tc, std::vector<int32_t>& need,
                        const char* item = "hypothesis") {
  if (hyp_off[0] != 0) return fail(CTCDEC_ERR_ARG, "hyp_off must start at 0");
  for (int32_t u = 0; u < n_utts; ++u) {
    if (hyp_off[u + 1] < hyp_off[u]) return fail(CTCDEC_ERR_ARG, "hyp_off must not decrease");
    if (int rc = check_frames(utt_logits, utt_frames, u)) return rc;
  }
  const int64_t NH = hyp_off[n_utts];
  if (NH > (int64_t)0x7FFFFFFF) return fail(CTCDEC_ERR_LIMIT, "more than 2^31 - 1 entries of hyp_off in one call");
  if (target_off[0] != 0) return fail(CTCDEC_ERR_ARG, "target_off must start at 0");
  need.assign((size_t)NH, 0);
  for (int32_t u = 0; u < n_utts; ++u)
    for (int64_t h = hyp_off[u]; h < hyp_off[u + 1]; ++h) {
      const std::string who = "utterance " + std::to_string(u) + ", " + item + " " + std::to_string(h - hyp_off[u]);
      const int64_t L = target_off[h + 1] - target_off[h];
      if (L < 0) return fail(CTCDEC_ERR_ARG, "target_off must not decrease");
      if (L > ALIGN_MAX_LABELS)
        return fail(CTCDEC_ERR_LIMIT, who + ": " + std::to_string(L) + " labels, above the limit of " + std::to_string(ALIGN_MAX_LABELS));
      if (L > 0 && !targets) return fail(CTCDEC_ERR_ARG, "no targets");
      int64_t nd = 0;
      if (int rc = check_labels(targets + target_off[h], L, tc.V, tc.blank, [&] { return who; }, "label", "label to score", nd)) return rc;
      need[(size_t)h] = (int32_t)nd;
    }
  return CTCDEC_OK;
}

// ---- items of utterances: what score, prefix scores, prefix sessions and phrase search share ----------------------------------
namespace {

// An utterance as the kernels' records name it
struct UttRows {
  const void* x = nullptr;      // (device) its matrix
  const double* lse = nullptr;  // (device) its rows' log-sum-exps
  int32_t T = 0, is_prob = 0;
};
static std::vector<UttRows> utt_rows(const AlignFront& fr, const std::vector<int64_t>& row0, const int32_t* utt_frames) {
  std::vector<UttRows> utts(fr.ptrs.size());
  for (size_t u = 0; u < utts.size(); ++u) utts[u] = UttRows{fr.ptrs[u], fr.lse + row0[u], utt_frames[u], fr.is_prob[u] ? 1 : 0};
  return utts;
}

// Where the items of a call go. Item h of utterance u (item_off[u] <= h < item_off[u + 1]) is launched when u has frames, and
// no fewer than need[h]: by the wave kernel up to wave_max labels (-1: the group kernel is forced), by the group kernel above.
// What an item that is not launched gets is its caller's decision. An utterance none of whose items is launched takes no
// part: use_frames has 0 for it, so that nothing of it is staged, classified or summed.
struct Routed {
  std::vector<int32_t> utt_of;      // [items] the item's utterance
  std::vector<int32_t> use_frames;  // [n_utts]
  std::vector<int32_t> run[2];      // the launched items in input order: [0] wave, [1] group
  bool any() const { return !run[0].empty() || !run[1].empty(); }
};
static Routed route_items(const int64_t* item_off, const int64_t* label_off, const int32_t* utt_frames, int32_t n_utts,
                          const std::vector<int32_t>& need, int32_t wave_max) {
  Routed r;
  r.utt_of.resize((size_t)item_off[n_utts]);
  r.use_frames.assign((size_t)n_utts, 0);
  for (int32_t u = 0; u < n_utts; ++u)
    for (int64_t h = item_off[u]; h < item_off[u + 1]; ++h) {
      r.utt_of[(size_t)h] = u;
      if (utt_frames[u] == 0 || utt_frames[u] < need[(size_t)h]) continue;
      r.run[label_off[h + 1] - label_off[h] <= wave_max ? 0 : 1].push_back((int32_t)h);
      r.use_frames[(size_t)u] = utt_frames[u];
    }
  return r;
}

// The forward pass of the items run[0] (wave kernel) and run[1] (group kernel), one launch each, longest utterance first inside
// it (run[] leaves in that order); the records of both go over in one copy. Item h's labels are w_alab[label_off[h] ..
// label_off[h + 1]) and its score goes to w_ascore[h]: the caller has uploaded the one and zeroed the other. ends: nullptr, or
// per item where its end states and their scale go (PrefixEnds).
static int forward_pass(ctcdec_decoder* dec, const TranscriptCall& tc, int32_t dtype, const std::vector<UttRows>& utts,
                        const std::vector<int32_t>& utt_of, const int64_t* label_off, std::vector<int32_t> (&run)[2],
                        const std::vector<PrefixEnds>* ends) {
  std::vector<ForwardHyp> hyps;
  std::vector<PrefixEnds> rec_l;
  int32_t max_chunks[2] = {1, 1};
  for (int w = 0; w < 2; ++w) {
    std::vector<int32_t>& g = run[w];
    std::stable_sort(g.begin(), g.end(), [&](int32_t a, int32_t b) { return utts[(size_t)utt_of[(size_t)a]].T > utts[(size_t)utt_of[(size_t)b]].T; });
    for (int32_t h : g) {
      const UttRows& u = utts[(size_t)utt_of[(size_t)h]];
      ForwardHyp a;
      a.x = u.x;
      a.lse = u.lse;
      a.lab = (const int32_t*)dec->w_alab.p + label_off[h];
      a.logp = (double*)dec->w_ascore.p + h;
      a.T = u.T;
      a.L = (int32_t)(label_off[h + 1] - label_off[h]);
      a.is_prob = u.is_prob;
      a.pad = 0;
      hyps.push_back(a);
      if (ends) rec_l.push_back((*ends)[(size_t)h]);
      max_chunks[w] = std::max(max_chunks[w], align_chunks(a.L));
    }
  }
  if (hyps.empty()) return CTCDEC_OK;
#ifdef CTC_SIM  // (both kernels are the one body here: a single thread owns every group)
  std::vector<double> col((size_t)2 * (size_t)std::max(max_chunks[0], max_chunks[1]));
  AlignSeqCtx cx;
  for (size_t i = 0; i < hyps.size(); ++i)
    for_dtype(dtype, [&](auto dt) {
      if (ends) ctc_forward_hyp<decltype(dt)::value, true>(cx, hyps[i], tc.V, tc.blank, tc.clip_lo, col.data(), &rec_l[i]);
      else ctc_forward_hyp<decltype(dt)::value>(cx, hyps[i], tc.V, tc.blank, tc.clip_lo, col.data());
    });
#else
  std::string err;
  if (upload(dec->w_fhyps, hyps, &err) || (ends && upload(dec->w_xrecl, rec_l, &err))) return fail(CTCDEC_ERR_DEVICE, err);
  for (int w = 0; w < 2; ++w) {
    const size_t first = w ? run[0].size() : 0;
    be::ForwardArgs fa;
    fa.hyps = (const ForwardHyp*)dec->w_fhyps.p + first;
    fa.n_hyps = (int32_t)run[w].size();
    fa.n_labels = tc.V;
    fa.dtype = dtype;
    fa.blank = tc.blank;
    fa.max_chunks = max_chunks[w];
    fa.pad = 0;
    fa.clip_lo = tc.clip_lo;
    if (ends ? be::launch_ctc_forward_ends(fa, (const PrefixEnds*)dec->w_xrecl.p + first, w == 0, &err)
             : be::launch_ctc_forward(fa, w == 0, &err))
      return fail(CTCDEC_ERR_DEVICE, err);
  }
#endif
  return CTCDEC_OK;
}

// Every label's score after the n_rows prefixes of a call, into `next` (out: next_out, the caller's device buffer, or the
// decoder's block): ctc_prefix_extend over the launched rows `rows` -- an utterance's next to each other, in the caller's
// order, utt_of[row] the utterance --, in chunks of up to PREFIX_K rows of one utterance. rec_h, last: per row of the call,
// where the forward pass stored its end states, and its last label (-1: none). dead: the rows nothing is launched for; they
// get -inf here when next is the caller's buffer, and are the caller's to fill on the host otherwise.
// In two steps, because every upload waits for the stream: stage() fills, forms the chunks and uploads; launch() launches.
// A caller whose forward pass comes with the call (ctcdec_prefix_batch) queues it between the two, behind every upload.
struct PrefixExtend {
  double* next = nullptr;
  int stage(ctcdec_decoder* dec, const TranscriptCall& tc, int32_t dtype, const std::vector<UttRows>& utts,
            const std::vector<int32_t>& utt_of, const std::vector<int32_t>& rows, const std::vector<PrefixEnds>& rec_h,
            const std::vector<int32_t>& last, const std::vector<int32_t>& dead, size_t n_rows, double* next_out);
  int launch();

 private:
  PrefixExtendArgs xa;
  std::vector<PrefixChunk> chunks;
};
int PrefixExtend::stage(ctcdec_decoder* dec, const TranscriptCall& tc, int32_t dtype, const std::vector<UttRows>& utts,
                        const std::vector<int32_t>& utt_of, const std::vector<int32_t>& rows, const std::vector<PrefixEnds>& rec_h,
                        const std::vector<int32_t>& last, const std::vector<int32_t>& dead, size_t n_rows, double* next_out) {
  std::string err;
  const int V = tc.V;
  next = next_out;
  if (!next) {
    if (dec->w_xnext.ensure(n_rows * (size_t)V * 8, &err)) return fail(CTCDEC_ERR_DEVICE, err);
    next = (double*)dec->w_xnext.p;
  }
  if (next_out && !dead.empty()) {
    if (upload(dec->w_xrows, dead, &err)) return fail(CTCDEC_ERR_DEVICE, err);
#ifdef CTC_SIM
    for (int32_t h : dead)
      for (int c = 0; c < V; ++c) next[(size_t)h * (size_t)V + (size_t)c] = align_neg_inf();
#else
    for (size_t at = 0; at < dead.size(); at += 65535) {
      const int32_t count = (int32_t)std::min<size_t>(65535, dead.size() - at);
      if (be::launch_ctc_prefix_fill(next, (const int32_t*)dec->w_xrows.p + at, count, V, &err)) return fail(CTCDEC_ERR_DEVICE, err);
    }
#endif
  }
  int32_t max_segs = 1;
  for (size_t at = 0; at < rows.size();) {
    const int32_t u = utt_of[(size_t)rows[at]];
    PrefixChunk ch{};
    ch.x = utts[(size_t)u].x;
    ch.lse = utts[(size_t)u].lse;
    ch.T = utts[(size_t)u].T;
    ch.is_prob = utts[(size_t)u].is_prob;
    for (; at < rows.size() && utt_of[(size_t)rows[at]] == u; ++at) {
      ch.h[ch.n++] = rows[at];
      if (ch.n == PREFIX_K) chunks.push_back(ch), ch.n = 0;
    }
    if (ch.n) chunks.push_back(ch);
    max_segs = std::max(max_segs, prefix_segments(ch.T));
  }
  if (chunks.empty()) return CTCDEC_OK;
  xa.n_chunks = (int32_t)chunks.size();
  xa.n_labels = V;
  xa.dtype = dtype;
  xa.blank = tc.blank;
  xa.max_segs = max_segs;
  xa.split = prefix_split((int64_t)chunks.size(), V) ? 1 : 0;
  xa.clip_lo = tc.clip_lo;
  const size_t part = xa.split ? chunks.size() * (size_t)max_segs * PREFIX_K * (size_t)V : 1;
  if (dec->w_xpart.ensure(part * 8, &err) || upload(dec->w_xrech, rec_h, &err) || upload(dec->w_xlast, last, &err) ||
      upload(dec->w_xchunks, chunks, &err))
    return fail(CTCDEC_ERR_DEVICE, err);
  xa.chunks = (const PrefixChunk*)dec->w_xchunks.p;
  xa.ends = (const PrefixEnds*)dec->w_xrech.p;
  xa.last = (const int32_t*)dec->w_xlast.p;
  xa.next = next;
  xa.partial = (double*)dec->w_xpart.p;
  return CTCDEC_OK;
}
int PrefixExtend::launch() {
  if (chunks.empty()) return CTCDEC_OK;
#ifdef CTC_SIM  // (a single thread owns, in turn, every column)
  AlignSeqCtx cx;
  std::vector<double> w((size_t)PREFIX_W_DOUBLES);
  for (int32_t k = 0; k < xa.n_chunks; ++k) {
    const int nseg = prefix_segments(chunks[(size_t)k].T);
    for (int c = 0; c < xa.n_labels; ++c) {
      for_dtype(xa.dtype, [&](auto dt) {
        if (!xa.split) return ctc_prefix_extend_tile<decltype(dt)::value>(cx, xa, k, c, 0, nseg, w.data());
        for (int seg = 0; seg < nseg; ++seg) ctc_prefix_extend_tile<decltype(dt)::value>(cx, xa, k, c, seg, seg + 1, w.data());
      });
      if (xa.split) ctc_prefix_finish_col(xa, k, c);
    }
  }
#else
  std::string err;
  if (be::launch_ctc_prefix_extend(xa, &err)) return fail(CTCDEC_ERR_DEVICE, err);
#endif
  return CTCDEC_OK;
}
}  // namespace

extern "C" {

int ctcdec_score_batch(ctcdec_decoder* dec, const void* const* utt_logits, const int32_t* utt_frames, int32_t n_utts, int32_t dtype,
                       int32_t is_device, const int32_t* targets, const int64_t* target_off, const int64_t* hyp_off, int32_t kernel,
                       double* logp_out, double* ms4, int64_t* launched2) {
  TranscriptCall tc;
  const bool args_ok = dec && n_utts >= 0 && target_off && hyp_off && (n_utts == 0 || (utt_logits && utt_frames));
  if (int rc = transcript_open(dec, args_ok, dtype, bad_kernel(kernel), tc)) return rc;
  std::vector<int32_t> need;
  if (int rc = check_scores(utt_logits, utt_frames, n_utts, targets, target_off, hyp_off, tc, need)) return rc;
  const size_t n = (size_t)n_utts;
  const int64_t NH = hyp_off[n];
  if (NH > 0 && !logp_out) return fail(CTCDEC_ERR_ARG, "no room for the scores");
  const auto t_begin = Clock::now();
  double tms[4] = {0, 0, 0, 0};
  int64_t launched[2] = {0, 0};
  // A hypothesis with fewer frames than labels plus adjacent equal labels has no alignment: probability 0, decided here.
  // The empty one without frames has the one empty alignment. Everything else goes to a kernel: the wave kernel up to its
  // limit (unless the group kernel is forced), the group kernel above it.
  Routed r = route_items(hyp_off, target_off, utt_frames, n_utts, need, kernel == 2 ? -1 : FORWARD_WAVE_MAX_LABELS);
  for (int64_t h = 0; h < NH; ++h) {
    const int32_t T = utt_frames[r.utt_of[(size_t)h]];
    if (T < need[(size_t)h]) logp_out[h] = align_neg_inf();
    else if (T == 0) logp_out[h] = 0.0;
  }
  if (r.any()) {
    const std::vector<int64_t> row0 = row_starts(r.use_frames.data(), n);
    const int64_t NL = target_off[NH];
    std::string err;
    AlignFront fr;
    if (int rc = align_front(dec, utt_logits, r.use_frames.data(), n_utts, dtype, is_device, tc.V, row0, fr)) return rc;
    tms[0] = fr.sniff_ms;
    if (dec->w_alab.ensure((size_t)std::max<int64_t>(NL, 1) * 4, &err) || dec->w_ascore.ensure((size_t)NH * 8, &err))
      return fail(CTCDEC_ERR_DEVICE, err);
    if ((NL && be::h2d(dec->w_alab.p, targets, (size_t)NL * 4, &err)) || be::zero(dec->w_ascore.p, (size_t)NH * 8, &err))
      return fail(CTCDEC_ERR_DEVICE, err);
    if (int rc = forward_pass(dec, tc, dtype, utt_rows(fr, row0, utt_frames), r.utt_of, target_off, r.run, nullptr)) return rc;
    for (int w = 0; w < 2; ++w) launched[w] = (int64_t)r.run[w].size();
    std::vector<double> got((size_t)NH);
    if (be::d2h(got.data(), dec->w_ascore.p, (size_t)NH * 8, &err)) return fail(CTCDEC_ERR_DEVICE, err);
    for (int w = 0; w < 2; ++w)
      for (int32_t h : r.run[w]) logp_out[h] = got[(size_t)h];
#ifndef CTC_SIM
    tms[1] = be::align_kernel_ms(be::K_ROW_LSE);
    tms[2] = be::align_kernel_ms(be::K_FORWARD);
#endif
  }
  tms[3] = ms(t_begin, Clock::now());
  if (ms4)
    for (int k = 0; k < 4; ++k) ms4[k] = tms[k];
  if (launched2) launched2[0] = launched[0], launched2[1] = launched[1];
  return CTCDEC_OK;
}

// ---- prefix scores ("Prefix scores") ----------------------------------------------------------------------------
}  // extern "C"

struct ctcdec_prefix {
  std::vector<double> end, next;  // [n_prefixes], [n_prefixes * V] (empty when the caller's device buffer took them)
  int32_t V = 0;
  bool next_with_caller = false;
  int32_t launches[3] = {0, 0, 0};  // row_lse, the forward kernels, ctc_prefix_extend / _finish / _fill
  int64_t launched[2] = {0, 0};
  double ms[5] = {0, 0, 0, 0, 0};
};

// The call behind ctcdec_prefix_batch: the checked prefixes (need[h]: labels plus adjacent equal labels) to a result.
static int prefix_call(ctcdec_decoder* dec, const TranscriptCall& tc, const void* const* utt_logits, const int32_t* utt_frames,
                       int32_t n_utts, int32_t dtype, int32_t is_device, const int32_t* labels, const int64_t* label_off,
                       const int64_t* prefix_off, const std::vector<int32_t>& need, int32_t kernel, double* next_out, ctcdec_prefix* res) {
  const size_t n = (size_t)n_utts;
  const int64_t NH = prefix_off[n];
  const int V = tc.V;
  const double NEG = align_neg_inf();
  res->V = V;
  res->next_with_caller = next_out != nullptr;
  res->end.assign((size_t)NH, NEG);
  if (NH == 0) return CTCDEC_OK;
  // A prefix with fewer frames than labels plus adjacent equal labels cannot be complete: end and next are -inf, decided
  // here. Without frames the empty prefix has the one empty alignment and nothing follows it. Everything else goes to a
  // forward kernel -- the wave kernel up to its limit (unless the group kernel is forced), the group kernel above it -- and
  // then, in chunks of PREFIX_K per utterance, to ctc_prefix_extend.
  Routed r = route_items(prefix_off, label_off, utt_frames, n_utts, need, kernel == 2 ? -1 : FORWARD_WAVE_MAX_LABELS);
  std::vector<int32_t> dead, live;  // no launch; launched, in input order
  for (int64_t h = 0; h < NH; ++h) {
    const int32_t T = utt_frames[r.utt_of[(size_t)h]];
    if (T >= need[(size_t)h] && T > 0) {
      live.push_back((int32_t)h);
      continue;
    }
    if (T >= need[(size_t)h]) res->end[(size_t)h] = 0.0;  // (no frames, no labels)
    dead.push_back((int32_t)h);
  }
  std::string err;
  const size_t next_count = (size_t)NH * (size_t)V;
  if (!next_out) res->next.assign(next_count, NEG);
  if (!r.any() && !next_out) return CTCDEC_OK;  // (the host's rows are filled already)
  const std::vector<int64_t> row0 = row_starts(r.use_frames.data(), n);
  const int64_t NL = label_off[NH];
  AlignFront fr;
  if (r.any()) {
    if (int rc = align_front(dec, utt_logits, r.use_frames.data(), n_utts, dtype, is_device, V, row0, fr)) return rc;
  } else if (int rc = device_only_front(fr)) {  // (only rows to fill: the device all the same)
    return rc;
  }
  std::vector<UttRows> utts;
  std::vector<PrefixEnds> rec_h;
  std::vector<int32_t> last;
  if (r.any()) {
    if (dec->w_alab.ensure((size_t)std::max<int64_t>(NL, 1) * 4, &err) || dec->w_ascore.ensure((size_t)NH * 8, &err) ||
        dec->w_xscale.ensure((size_t)NH * 8, &err))
      return fail(CTCDEC_ERR_DEVICE, err);
    if ((NL && be::h2d(dec->w_alab.p, labels, (size_t)NL * 4, &err)) || be::zero(dec->w_ascore.p, (size_t)NH * 8, &err))
      return fail(CTCDEC_ERR_DEVICE, err);
    // where each launched prefix' 2 T end states go, and every prefix' last label
    int64_t n_ends = 0;
    for (int32_t h : live) n_ends += 2 * (int64_t)utt_frames[r.utt_of[(size_t)h]];
    if (dec->w_xends.ensure((size_t)n_ends * 8, &err)) return fail(CTCDEC_ERR_DEVICE, err);
    rec_h.assign((size_t)NH, PrefixEnds{nullptr, nullptr});
    last.assign((size_t)NH, -1);
    for (int64_t h = 0; h < NH; ++h)
      if (label_off[h + 1] > label_off[h]) last[(size_t)h] = labels[label_off[h + 1] - 1];
    n_ends = 0;
    for (int32_t h : live) {
      rec_h[(size_t)h] = PrefixEnds{(double*)dec->w_xends.p + n_ends, (double*)dec->w_xscale.p + h};
      n_ends += 2 * (int64_t)utt_frames[r.utt_of[(size_t)h]];
    }
    utts = utt_rows(fr, row0, utt_frames);
  }
  // the rows nothing is launched for (on the device; a host caller's were filled above) and the extend step's uploads, the
  // forward launches as ctcdec_score_batch makes them, the extend launch
  PrefixExtend px;
  if (int rc = px.stage(dec, tc, dtype, utts, r.utt_of, live, rec_h, last, dead, (size_t)NH, next_out)) return rc;
  if (r.any()) {
    if (int rc = forward_pass(dec, tc, dtype, utts, r.utt_of, label_off, r.run, &rec_h)) return rc;
    for (int w = 0; w < 2; ++w) res->launched[w] = (int64_t)r.run[w].size();
    if (int rc = px.launch()) return rc;
    std::vector<double> got((size_t)NH);
    if (be::d2h(got.data(), dec->w_ascore.p, (size_t)NH * 8, &err)) return fail(CTCDEC_ERR_DEVICE, err);
    for (int32_t h : live) res->end[(size_t)h] = got[(size_t)h];
    if (!next_out) {
      // the launched rows come back; the others keep the host's -inf (nothing wrote them on the device)
      std::vector<double> back(next_count);
      if (be::d2h(back.data(), px.next, next_count * 8, &err)) return fail(CTCDEC_ERR_DEVICE, err);
      for (int32_t h : live)
        std::copy(back.begin() + (size_t)h * (size_t)V, back.begin() + ((size_t)h + 1) * (size_t)V, res->next.begin() + (size_t)h * (size_t)V);
    }
  }
  if (be::sync(&err)) return fail(CTCDEC_ERR_DEVICE, err);
#ifndef CTC_SIM
  if (r.any()) {
    res->ms[0] = be::last_prune_ms();
    res->ms[1] = be::align_kernel_ms(be::K_ROW_LSE);
    res->ms[2] = be::align_kernel_ms(be::K_FORWARD);
    res->launches[0] = be::align_kernel_launches(be::K_ROW_LSE);
    res->launches[1] = be::align_kernel_launches(be::K_FORWARD);
  }
  res->ms[3] = be::align_kernel_ms(be::K_PREFIX_EXTEND);
  res->launches[2] = be::align_kernel_launches(be::K_PREFIX_EXTEND);
#endif
  return CTCDEC_OK;
}

extern "C" {

int ctcdec_prefix_batch(ctcdec_decoder* dec, const void* const* utt_logits, const int32_t* utt_frames, int32_t n_utts, int32_t dtype,
                        int32_t is_device, const int32_t* labels, const int64_t* label_off, const int64_t* prefix_off, int32_t kernel,
                        double* next_out, ctcdec_prefix** out) {
  TranscriptCall tc;
  const bool args_ok = dec && out && n_utts >= 0 && label_off && prefix_off && (n_utts == 0 || (utt_logits && utt_frames));
  if (int rc = transcript_open(dec, args_ok, dtype, bad_kernel(kernel), tc)) return rc;
  std::vector<int32_t> need;
  if (int rc = check_scores(utt_logits, utt_frames, n_utts, labels, label_off, prefix_off, tc, need, "prefix")) return rc;
  if (next_out && !is_device) return fail(CTCDEC_ERR_ARG, "a buffer for next is device memory: it goes with device logits");
  if (prefix_off[n_utts] * (int64_t)tc.V > (int64_t)1 << 40) return fail(CTCDEC_ERR_LIMIT, "more than 2^40 prefix scores in one call");
  const auto t_begin = Clock::now();
  std::unique_ptr<ctcdec_prefix> res(new ctcdec_prefix);
  if (int rc = prefix_call(dec, tc, utt_logits, utt_frames, n_utts, dtype, is_device, labels, label_off, prefix_off, need, kernel, next_out,
                           res.get()))
    return rc;
  res->ms[4] = ms(t_begin, Clock::now());
  *out = res.release();
  return CTCDEC_OK;
}

int ctcdec_prefix_scores(const ctcdec_prefix* p, const double** end_out, const double** next_out, int64_t* n_prefixes_out,
                         int32_t* n_labels_out) {
  if (!p || !end_out || !next_out || !n_prefixes_out || !n_labels_out) return fail(CTCDEC_ERR_ARG, "no prefix result");
  *end_out = p->end.data();
  *next_out = p->next_with_caller ? nullptr : p->next.data();
  *n_prefixes_out = (int64_t)p->end.size();
  *n_labels_out = p->V;
  return CTCDEC_OK;
}

int ctcdec_prefix_timing(const ctcdec_prefix* p, double* ms5, int32_t* launches3, int64_t* launched2) {
  if (!p || !ms5) return fail(CTCDEC_ERR_ARG, "no prefix result");
  for (int k = 0; k < 5; ++k) ms5[k] = p->ms[k];
  if (launches3)
    for (int k = 0; k < 3; ++k) launches3[k] = p->launches[k];
  if (launched2) launched2[0] = p->launched[0], launched2[1] = p->launched[1];
  return CTCDEC_OK;
}

void ctcdec_prefix_free(ctcdec_prefix* p) { delete p; }

// ---- prefix sessions ("Prefix sessions") ------------------------------------------------------------------------
}  // extern "C"

// What outlives a call: the batch's row log-sum-exps, classification and (host input) staged matrices, and an arena of
// `capacity` slots of 2 * T_max end states plus a scale. Slot s < n_utts is the root of utterance s. An id is a slot under
// the tag it was handed out with; tags come from one counter for all sessions, so a stale id and another session's id
// both fail the same test.
struct ctcdec_prefix_session {
  ctcdec_decoder* dec = nullptr;
  TranscriptCall tc;
  int32_t n_utts = 0, dtype = 0, T_max = 0;
  bool is_device = false;
  int64_t capacity = 0;
  std::vector<UttRows> utts;  // (x: the caller's tensors, or rows of `logits`; lse: rows of `lse`)
  DevBuf logits, lse, arena, scales;
  std::vector<uint32_t> tag;      // per slot: 0 while free
  std::vector<int32_t> utt, last, len;
  std::vector<int64_t> free_slots;  // taken from the back: the lowest slot first
  double ms[3] = {0, 0, 0};
  int32_t launches[4] = {0, 0, 0, 0};
  double* bc(int64_t slot) const { return (double*)arena.p + (size_t)slot * 2 * (size_t)T_max; }
  double* scale(int64_t slot) const { return (double*)scales.p + slot; }
};

static uint32_t g_session_tag = 0;  // (under the device lock)
static uint32_t session_next_tag() {
  if (++g_session_tag == 0) ++g_session_tag;
  return g_session_tag;
}
static int64_t session_id(uint32_t tag, int64_t slot) { return (int64_t)(((uint64_t)tag << 31) | (uint64_t)slot); }
// The slot of a live id, -1 for anything else
static int64_t session_slot(const ctcdec_prefix_session* s, int64_t id) {
  if (id < 0) return -1;
  const int64_t slot = id & (int64_t)0x7FFFFFFF;
  const uint32_t tag = (uint32_t)((uint64_t)id >> 31);
  return slot < s->capacity && tag != 0 && s->tag[(size_t)slot] == tag ? slot : -1;
}

// The second half of an open or an extend: the call's prefixes are slots[i], in the caller's order, their end states and
// scales in the arena and their `end` in dec->w_ascore[i] (device). Every label's score by ctc_prefix_extend, in chunks of up
// to PREFIX_K prefixes of one utterance, into next_out (device) or the decoder's block and from there into next_host; `end`
// into end_out. An utterance without frames launches nothing: its empty prefix has end 0.0, every other -inf, next is -inf.
static int session_deliver(ctcdec_prefix_session* s, const std::vector<int64_t>& slots, double* next_out, double* end_out,
                           double* next_host) {
  ctcdec_decoder* dec = s->dec;
  const int V = s->tc.V;
  const double NEG = align_neg_inf();
  const size_t n = slots.size();
  if (n == 0) return CTCDEC_OK;
  std::string err;
  std::vector<PrefixEnds> rec_h(n, PrefixEnds{nullptr, nullptr});
  std::vector<int32_t> last(n, -1), utt_of(n), dead, order;
  for (size_t i = 0; i < n; ++i) {
    const int64_t slot = slots[i];
    last[i] = s->last[(size_t)slot];
    utt_of[i] = s->utt[(size_t)slot];
    if (s->utts[(size_t)utt_of[i]].T == 0) {
      dead.push_back((int32_t)i);
      continue;
    }
    rec_h[i] = PrefixEnds{s->bc(slot), s->scale(slot)};
    order.push_back((int32_t)i);
  }
  // an utterance's prefixes of the call next to each other, in the caller's order
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return utt_of[(size_t)a] < utt_of[(size_t)b]; });
  PrefixExtend px;
  if (int rc = px.stage(dec, s->tc, s->dtype, s->utts, utt_of, order, rec_h, last, dead, n, next_out)) return rc;
  if (int rc = px.launch()) return rc;
  std::vector<double> got(n, NEG);
  if (!order.empty() && be::d2h(got.data(), dec->w_ascore.p, n * 8, &err)) return fail(CTCDEC_ERR_DEVICE, err);
  if (next_host) {
    if (!order.empty() && be::d2h(next_host, px.next, n * (size_t)V * 8, &err)) return fail(CTCDEC_ERR_DEVICE, err);
    for (int32_t h : dead) std::fill(next_host + (size_t)h * (size_t)V, next_host + ((size_t)h + 1) * (size_t)V, NEG);
  }
  for (int32_t h : dead) got[(size_t)h] = s->len[(size_t)slots[(size_t)h]] == 0 ? 0.0 : NEG;
  std::copy(got.begin(), got.end(), end_out);
  if (be::sync(&err)) return fail(CTCDEC_ERR_DEVICE, err);
  return CTCDEC_OK;
}

// The timers and launch counts of the call that ends here (the kernels' event logs since the call's reset)
static void session_timing(ctcdec_prefix_session* s, Clock::time_point t_begin, int32_t sim_advances) {
#ifdef CTC_SIM
  s->ms[0] = s->ms[1] = 0;
  s->launches[0] = sim_advances;  // (the simulator runs the body over all children once: counted as the one launch it stands for)
  s->launches[1] = s->launches[2] = s->launches[3] = 0;
#else
  (void)sim_advances;
  s->ms[0] = be::align_kernel_ms(be::K_PREFIX_ADVANCE);
  s->ms[1] = be::align_kernel_ms(be::K_PREFIX_EXTEND);
  s->launches[0] = be::align_kernel_launches(be::K_PREFIX_ADVANCE);
  s->launches[1] = be::align_kernel_launches(be::K_PREFIX_EXTEND);
  s->launches[2] = be::align_kernel_launches(be::K_ROW_LSE);
  s->launches[3] = be::align_kernel_launches(be::K_FORWARD);
#endif
  s->ms[2] = ms(t_begin, Clock::now());
}

extern "C" {

int ctcdec_prefix_session_open(ctcdec_decoder* dec, const void* const* utt_logits, const int32_t* utt_frames, int32_t n_utts,
                               int32_t dtype, int32_t is_device, int64_t capacity, double* next_out, int64_t* root_ids,
                               double* root_end, double* next_host, ctcdec_prefix_session** out) {
  TranscriptCall tc;
  const bool args_ok = dec && out && n_utts >= 0 && (n_utts == 0 || (utt_logits && utt_frames && root_ids && root_end));
  if (int rc = transcript_open(dec, args_ok, dtype, "", tc)) return rc;
  const size_t n = (size_t)n_utts;
  int32_t T_max = 0;
  for (int32_t u = 0; u < n_utts; ++u) {
    if (int rc = check_frames(utt_logits, utt_frames, u)) return rc;
    T_max = std::max(T_max, utt_frames[u]);
  }
  if (capacity < n_utts)
    return fail(CTCDEC_ERR_ARG, "a session needs a slot for every utterance's empty prefix: capacity " + std::to_string(capacity) +
                                    " for " + std::to_string(n_utts) + " utterances");
  if (capacity > (int64_t)0x7FFFFFFF) return fail(CTCDEC_ERR_LIMIT, "more than 2^31 - 1 slots in one session");
  if (next_out && !is_device) return fail(CTCDEC_ERR_ARG, "a buffer for next is device memory: it goes with device logits");
  if (n_utts > 0 && !next_out && !next_host) return fail(CTCDEC_ERR_ARG, "no room for the roots' next");
  const auto t_begin = Clock::now();
  std::unique_ptr<ctcdec_prefix_session> s(new ctcdec_prefix_session);
  s->dec = dec, s->tc = tc, s->n_utts = n_utts, s->dtype = dtype, s->T_max = T_max, s->is_device = is_device != 0, s->capacity = capacity;
  const std::vector<int64_t> row0 = row_starts(utt_frames, n);
  const int64_t R = row0[n];
  const int V = tc.V;
  std::string err;
  AlignFront fr;
  if (R > 0) {
    if (int rc = align_front(dec, utt_logits, utt_frames, n_utts, dtype, is_device, V, row0, fr)) return rc;
  } else {  // (no frames at all: nothing to stage, classify or sum)
    if (int rc = device_only_front(fr)) return rc;
    fr.ptrs.assign(n, nullptr);
    fr.is_prob.assign(n, 0);
  }
  // what must outlive this call leaves the decoder's workspaces
  const size_t row_bytes = (size_t)V * dtype_size(dtype);
  if (s->lse.ensure((size_t)std::max<int64_t>(R, 1) * 8, &err) || s->arena.ensure(std::max<size_t>((size_t)capacity * 2 * (size_t)T_max * 8, 16), &err) ||
      s->scales.ensure(std::max<size_t>((size_t)capacity * 8, 16), &err))
    return fail(CTCDEC_ERR_DEVICE, err);
  if (R > 0 && be::d2d(s->lse.p, fr.lse, (size_t)R * 8, &err)) return fail(CTCDEC_ERR_DEVICE, err);
  const bool own_logits = !is_device && R > 0;
  if (own_logits && (s->logits.ensure((size_t)R * row_bytes, &err) || be::d2d(s->logits.p, dec->w_logits.p, (size_t)R * row_bytes, &err)))
    return fail(CTCDEC_ERR_DEVICE, err);
  s->utts.resize(n);
  for (size_t u = 0; u < n; ++u) {
    const void* x = own_logits ? (const char*)s->logits.p + (size_t)row0[u] * row_bytes : fr.ptrs[u];
    s->utts[u] = UttRows{x, (const double*)s->lse.p + row0[u], utt_frames[u], fr.is_prob[u] ? 1 : 0};
  }
  s->tag.assign((size_t)capacity, 0);
  s->utt.assign((size_t)capacity, -1);
  s->last.assign((size_t)capacity, -1);
  s->len.assign((size_t)capacity, 0);
  for (int64_t slot = capacity - 1; slot >= n_utts; --slot) s->free_slots.push_back(slot);
  std::vector<int64_t> roots(n);
  for (size_t u = 0; u < n; ++u) {
    roots[u] = (int64_t)u;
    s->tag[u] = session_next_tag();
    s->utt[u] = (int32_t)u;
    root_ids[u] = session_id(s->tag[u], (int64_t)u);
  }
  // the roots' end states: the forward pass of the empty prefix (item u: utterance u's, without labels), by the wave kernel
  if (dec->w_alab.ensure(4, &err) || dec->w_ascore.ensure(std::max<size_t>(n * 8, 16), &err) || be::zero(dec->w_ascore.p, std::max<size_t>(n * 8, 16), &err))
    return fail(CTCDEC_ERR_DEVICE, err);
  std::vector<int32_t> utt_of(n), run[2];
  std::vector<PrefixEnds> ends(n);
  const std::vector<int64_t> label_off(n + 1, 0);
  for (size_t u = 0; u < n; ++u) {
    utt_of[u] = (int32_t)u;
    ends[u] = PrefixEnds{s->bc((int64_t)u), s->scale((int64_t)u)};
    if (utt_frames[u] > 0) run[0].push_back((int32_t)u);
  }
  if (int rc = forward_pass(dec, tc, dtype, s->utts, utt_of, label_off.data(), run, &ends)) return rc;
  if (int rc = session_deliver(s.get(), roots, next_out, root_end, next_host)) return rc;
  session_timing(s.get(), t_begin, 0);
  *out = s.release();
  return CTCDEC_OK;
}

int ctcdec_prefix_session_extend(ctcdec_prefix_session* s, const int64_t* parents, const int32_t* labels, int64_t n, double* next_out,
                                 int64_t* ids_out, double* end_out, double* next_host) {
  if (!s || n < 0 || (n > 0 && (!parents || !labels || !ids_out || !end_out))) return fail(CTCDEC_ERR_ARG, "bad arguments");
  if (next_out && !s->is_device) return fail(CTCDEC_ERR_ARG, "a buffer for next is device memory: it goes with device logits");
  if (n > 0 && !next_out && !next_host) return fail(CTCDEC_ERR_ARG, "no room for next");
  std::lock_guard<std::mutex> device_lock(g_device_mu);
  const auto t_begin = Clock::now();
  ctcdec_decoder* dec = s->dec;
  const int V = s->tc.V;
  // everything before anything is launched or taken
  std::vector<int64_t> pslot((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    const std::string who = "child " + std::to_string(i);
    const int64_t p = session_slot(s, parents[i]);
    if (p < 0) return fail(CTCDEC_ERR_ARG, who + ": parent " + std::to_string(parents[i]) + " is not a live prefix of this session");
    if (labels[i] < 0 || labels[i] >= V) return fail(CTCDEC_ERR_ARG, who + ": label " + std::to_string(labels[i]) + " is outside the alphabet");
    if (labels[i] == s->tc.blank) return fail(CTCDEC_ERR_ARG, who + ": the blank is not a label to extend by");
    if (s->len[(size_t)p] + 1 > ALIGN_MAX_LABELS)
      return fail(CTCDEC_ERR_LIMIT, who + ": " + std::to_string(s->len[(size_t)p] + 1) + " labels, above the limit of " + std::to_string(ALIGN_MAX_LABELS));
    pslot[(size_t)i] = p;
  }
  if ((int64_t)s->free_slots.size() < n)
    return fail(CTCDEC_ERR_LIMIT, std::to_string(n) + " children for " + std::to_string(s->free_slots.size()) + " free slots of " +
                                      std::to_string(s->capacity) + ": release prefixes, or open the session with a larger capacity");
  if (n == 0) {
    session_timing(s, t_begin, 0);
    return CTCDEC_OK;
  }
  std::string err;
  if (be::bind_thread(&err)) return fail(CTCDEC_ERR_DEVICE, err);
#ifndef CTC_SIM
  be::align_timing_reset();
#endif
  // the children's slots (not handed out before the call has succeeded), and their records: an utterance's next to each other
  std::vector<int64_t> slots((size_t)n);
  for (int64_t i = 0; i < n; ++i) slots[(size_t)i] = s->free_slots[s->free_slots.size() - 1 - (size_t)i];
  std::vector<int32_t> order;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t slot = slots[(size_t)i], p = pslot[(size_t)i];
    s->utt[(size_t)slot] = s->utt[(size_t)p];
    s->last[(size_t)slot] = labels[i];
    s->len[(size_t)slot] = s->len[(size_t)p] + 1;
    if (s->utts[(size_t)s->utt[(size_t)p]].T > 0) order.push_back((int32_t)i);
  }
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return s->utt[(size_t)slots[(size_t)a]] < s->utt[(size_t)slots[(size_t)b]]; });
  std::vector<PrefixChild> kids;
  kids.reserve(order.size());
  if (dec->w_ascore.ensure((size_t)n * 8, &err) || be::zero(dec->w_ascore.p, (size_t)n * 8, &err)) return fail(CTCDEC_ERR_DEVICE, err);
  for (int32_t i : order) {
    const int64_t slot = slots[(size_t)i], p = pslot[(size_t)i];
    const int32_t u = s->utt[(size_t)slot];
    PrefixChild k;
    k.x = s->utts[(size_t)u].x;
    k.lse = s->utts[(size_t)u].lse;
    k.parent = s->bc(p);
    k.bc = s->bc(slot);
    k.scale = s->scale(slot);
    k.end = (double*)dec->w_ascore.p + i;
    k.T = s->utts[(size_t)u].T;
    k.c = labels[i];
    k.parent_last = s->last[(size_t)p];
    k.is_prob = s->utts[(size_t)u].is_prob;
    kids.push_back(k);
  }
#ifdef CTC_SIM
  for_dtype(s->dtype, [&](auto dt) {
    for (const PrefixChild& k : kids) ctc_prefix_advance_child<decltype(dt)::value>(k, V, s->tc.blank, s->tc.clip_lo);
  });
#else
  if (!kids.empty()) {
    if (upload(dec->w_fhyps, kids, &err)) return fail(CTCDEC_ERR_DEVICE, err);
    PrefixAdvanceArgs aa;
    aa.kids = (const PrefixChild*)dec->w_fhyps.p;
    aa.n_kids = (int32_t)kids.size();
    aa.n_labels = V;
    aa.dtype = s->dtype;
    aa.blank = s->tc.blank;
    aa.clip_lo = s->tc.clip_lo;
    if (be::launch_ctc_prefix_advance(aa, &err)) return fail(CTCDEC_ERR_DEVICE, err);
  }
#endif
  if (int rc = session_deliver(s, slots, next_out, end_out, next_host)) return rc;
  for (int64_t i = 0; i < n; ++i) {
    s->tag[(size_t)slots[(size_t)i]] = session_next_tag();
    ids_out[i] = session_id(s->tag[(size_t)slots[(size_t)i]], slots[(size_t)i]);
  }
  s->free_slots.resize(s->free_slots.size() - (size_t)n);
  session_timing(s, t_begin, kids.empty() ? 0 : 1);
  return CTCDEC_OK;
}

int ctcdec_prefix_session_release(ctcdec_prefix_session* s, const int64_t* ids, int64_t n) {
  if (!s || n < 0 || (n > 0 && !ids)) return fail(CTCDEC_ERR_ARG, "bad arguments");
  std::lock_guard<std::mutex> device_lock(g_device_mu);
  std::vector<int64_t> slots((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    const int64_t slot = session_slot(s, ids[i]);
    if (slot < 0) return fail(CTCDEC_ERR_ARG, "release: " + std::to_string(ids[i]) + " is not a live prefix of this session");
    if (slot < s->n_utts)
      return fail(CTCDEC_ERR_ARG, "release: " + std::to_string(ids[i]) + " is the empty prefix of utterance " + std::to_string(slot) +
                                      ", which lives as long as the session");
    slots[(size_t)i] = slot;
  }
  std::vector<int64_t> sorted = slots;
  std::sort(sorted.begin(), sorted.end());
  if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return fail(CTCDEC_ERR_ARG, "release: an id is given twice");
  for (int64_t slot : slots) {
    s->tag[(size_t)slot] = 0;
    s->free_slots.push_back(slot);
  }
  return CTCDEC_OK;
}

int ctcdec_prefix_session_timing(const ctcdec_prefix_session* s, double* ms3, int32_t* launches4) {
  if (!s || !ms3) return fail(CTCDEC_ERR_ARG, "no prefix session");
  std::lock_guard<std::mutex> device_lock(g_device_mu);
  for (int k = 0; k < 3; ++k) ms3[k] = s->ms[k];
  if (launches4)
    for (int k = 0; k < 4; ++k) launches4[k] = s->launches[k];
  return CTCDEC_OK;
}

void ctcdec_prefix_session_close(ctcdec_prefix_session* s) {
  if (!s) return;
  std::lock_guard<std::mutex> device_lock(g_device_mu);
  delete s;
}

// ---- frame posteriors ("Frame posteriors") --------------------------------------------------------------------
}  // extern "C"

struct ctcdec_posteriors {
  std::vector<int64_t> tok_off, gamma_off;
  std::vector<int32_t> gamma_stride;
  std::vector<double> logp, logp_backward, occupancy, centre, gamma;
  bool dense = false;
  int32_t launches = 0;
  int64_t launched[2] = {0, 0};
  double ms[4] = {0, 0, 0, 0};
};

// The tables of one ctc_posteriors launch (32 * frames * align_chunks(L) bytes per utterance) when the caller names no budget:
// about 640 utterances of 1000 frames and 100 labels, more than two workgroups for each of the device's 256 compute units,
// and under 1.5 % of its memory
static const int64_t POSTERIORS_TABLE_BUDGET = (int64_t)4 << 30;

static int64_t posteriors_table_bytes(int64_t T, int64_t L) { return 32 * T * (int64_t)align_chunks((int32_t)L); }

// What ctcdec_posteriors_batch and ctcdec_gradient_batch check before anything moves: labels, frame counts and feasibility
// are ctcdec_align_batch's; the budget is these calls' own
static int check_posteriors(const void* const* utt_logits, const int32_t* utt_frames, int32_t n_utts, const int64_t* label_off,
                            const int32_t* labels, int64_t budget, const TranscriptCall& tc) {
  if (int rc = check_alignment(utt_logits, utt_frames, n_utts, labels, label_off, INT64_MAX, tc)) return rc;
  for (int32_t u = 0; u < n_utts; ++u) {
    const int64_t bytes = posteriors_table_bytes(utt_frames[u], label_off[u + 1] - label_off[u]);
    if (bytes > budget)
      return fail(CTCDEC_ERR_LIMIT, "utterance " + std::to_string(u) + ": a table of " + std::to_string(bytes) + " bytes, above the budget of " +
                                        std::to_string(budget) + " bytes for one launch");
  }
  return CTCDEC_OK;
}

// One launch of ctc_posteriors over the utterances `g` of a call (at most two kernel launches: inside a launch the short
// targets, 256 threads, come before the long ones, 1024, longest utterance first in each; `g` leaves in that order). The
// call has uploaded its labels to w_alab and zeroed w_pocc and w_ascore. tab_off[j]: where utterance g[j]'s table starts in
// w_ptab, in doubles; count: the utterances each instantiation took; launches: kernel launches made.
struct PosteriorsLaunch {
  std::vector<int64_t> tab_off;
  int32_t count[2] = {0, 0};
  int32_t launches = 0;
};
static int posteriors_launch(ctcdec_decoder* dec, std::vector<int32_t>& g, const AlignFront& fr, const std::vector<int64_t>& row0,
                             const int32_t* utt_frames, const int64_t* label_off, int64_t NL, const TranscriptCall& tc, int32_t dtype,
                             int32_t dense, PosteriorsLaunch& out) {
  std::string err;
  std::stable_sort(g.begin(), g.end(), [&](int32_t a, int32_t b) {
    const bool la = align_chunks((int32_t)(label_off[a + 1] - label_off[a])) > ALIGN_THREADS;
    const bool lb = align_chunks((int32_t)(label_off[b + 1] - label_off[b])) > ALIGN_THREADS;
    return la != lb ? lb : utt_frames[a] > utt_frames[b];
  });
  std::vector<PostUtt> utts;
  std::vector<int64_t>& tab_off = out.tab_off;
  tab_off.clear();
  int64_t off = 0;
  int32_t max_chunks[2] = {1, 1};
  int32_t* count = out.count;
  count[0] = count[1] = 0;
  out.launches = 0;
  for (int32_t u : g) {
    const int32_t L = (int32_t)(label_off[u + 1] - label_off[u]);
    PostUtt a;
    a.x = fr.ptrs[(size_t)u];
    a.lse = fr.lse + row0[(size_t)u];
    a.lab = (const int32_t*)dec->w_alab.p + label_off[u];
    a.table = (double*)dec->w_ptab.p + off;
    a.logp = (double*)dec->w_ascore.p + 2 * (size_t)u;
    a.occ = (double*)dec->w_pocc.p + label_off[u];
    a.centre = (double*)dec->w_pocc.p + NL + label_off[u];
    a.T = utt_frames[u];
    a.L = L;
    a.is_prob = fr.is_prob[(size_t)u] ? 1 : 0;
    a.pad = 0;
    utts.push_back(a);
    tab_off.push_back(off);
    off += posteriors_table_bytes(utt_frames[u], L) / 8;
    const int w = align_chunks(L) > ALIGN_THREADS ? 1 : 0;
    max_chunks[w] = std::max(max_chunks[w], align_chunks(L));
    ++count[w];
  }
#ifdef CTC_SIM  // (the kernel's body: a single thread owns every group)
  std::vector<double> col((size_t)4 * (size_t)std::max(max_chunks[0], max_chunks[1]) + 2);
  AlignSeqCtx cx;
  for (const PostUtt& a : utts)
    for_dtype(dtype, [&](auto dt) { ctc_posteriors_utt<decltype(dt)::value>(cx, a, tc.V, tc.blank, tc.clip_lo, dense, col.data()); });
  for (int w = 0; w < 2; ++w) out.launches += count[w] ? 1 : 0;
#else
  if (upload(dec->w_putts, utts, &err)) return fail(CTCDEC_ERR_DEVICE, err);
  for (int w = 0; w < 2; ++w) {
    if (!count[w]) continue;
    be::PosteriorsArgs pa;
    pa.utts = (const PostUtt*)dec->w_putts.p + (w ? count[0] : 0);
    pa.n_utts = count[w];
    pa.n_labels = tc.V;
    pa.dtype = dtype;
    pa.blank = tc.blank;
    pa.max_chunks = max_chunks[w];
    pa.dense = dense ? 1 : 0;
    pa.clip_lo = tc.clip_lo;
    if (be::launch_ctc_posteriors(pa, &err)) return fail(CTCDEC_ERR_DEVICE, err);
    ++out.launches;
  }
#endif
  return CTCDEC_OK;
}

// What ctcdec_posteriors_batch and ctcdec_gradient_batch do between their checks and their launches: the device front, the
// labels uploaded, the token sums and the scores zeroed, the launches' utterances, and room for the largest launch's tables
static int posteriors_front(ctcdec_decoder* dec, const TranscriptCall& tc, const void* const* utt_logits, const int32_t* utt_frames,
                            int32_t n_utts, int32_t dtype, int32_t is_device, const int64_t* label_off, const int32_t* labels,
                            int64_t budget, const std::vector<int64_t>& row0, AlignFront& fr, std::vector<std::vector<int32_t>>& groups) {
  std::string err;
  if (int rc = align_front(dec, utt_logits, utt_frames, n_utts, dtype, is_device, tc.V, row0, fr)) return rc;
  const size_t n = (size_t)n_utts;
  const int64_t NL = label_off[n];
  const size_t nl1 = (size_t)std::max<int64_t>(NL, 1);
  if (dec->w_alab.ensure(nl1 * 4, &err) || dec->w_pocc.ensure(nl1 * 16, &err) || dec->w_ascore.ensure(n * 16, &err))
    return fail(CTCDEC_ERR_DEVICE, err);
  if ((NL && be::h2d(dec->w_alab.p, labels, (size_t)NL * 4, &err)) || be::zero(dec->w_pocc.p, nl1 * 16, &err) ||
      be::zero(dec->w_ascore.p, n * 16, &err))
    return fail(CTCDEC_ERR_DEVICE, err);
  const auto bytes_of = [&](int32_t u) { return posteriors_table_bytes(utt_frames[u], label_off[u + 1] - label_off[u]); };
  const int64_t most = budget_groups(n_utts, bytes_of, budget, groups);
  if (dec->w_ptab.ensure((size_t)std::max<int64_t>(most, 32), &err)) return fail(CTCDEC_ERR_DEVICE, err);
  return CTCDEC_OK;
}

extern "C" {

int ctcdec_posteriors_batch(ctcdec_decoder* dec, const void* const* utt_logits, const int32_t* utt_frames, int32_t n_utts, int32_t dtype,
                            int32_t is_device, const int64_t* label_off, const int32_t* labels, int32_t dense, int64_t table_budget,
                            ctcdec_posteriors** out) {
  TranscriptCall tc;
  const bool args_ok = dec && out && n_utts >= 0 && label_off && table_budget >= 0 && (n_utts == 0 || (utt_logits && utt_frames));
  if (int rc = transcript_open(dec, args_ok, dtype, "", tc)) return rc;
  const int64_t budget = table_budget ? table_budget : POSTERIORS_TABLE_BUDGET;
  if (int rc = check_posteriors(utt_logits, utt_frames, n_utts, label_off, labels, budget, tc)) return rc;
  const auto t_begin = Clock::now();
  std::unique_ptr<ctcdec_posteriors> res(new ctcdec_posteriors());
  const size_t n = (size_t)n_utts;
  const int64_t NL = label_off[n];
  const std::vector<int64_t> row0 = row_starts(utt_frames, n);
  const int64_t R = row0[n];
  res->dense = dense != 0;
  res->tok_off.assign(label_off, label_off + n + 1);
  res->logp.assign(n, 0.0);  // (no frames and the empty target: the one empty alignment)
  res->logp_backward.assign(n, 0.0);
  res->occupancy.assign((size_t)NL, 0.0);
  res->centre.assign((size_t)NL, 0.0);
  res->gamma_off.assign(n + 1, 0);
  res->gamma_stride.assign(n, 0);
  for (size_t u = 0; u < n; ++u) {
    res->gamma_stride[u] = 4 * align_chunks((int32_t)(label_off[u + 1] - label_off[u]));
    res->gamma_off[u + 1] = res->gamma_off[u] + (dense ? (int64_t)utt_frames[u] * res->gamma_stride[u] : 0);
  }
  if (dense) res->gamma.resize((size_t)res->gamma_off[n]);
  if (R > 0) {
    std::string err;
    AlignFront fr;
    std::vector<std::vector<int32_t>> groups;
    if (int rc = posteriors_front(dec, tc, utt_logits, utt_frames, n_utts, dtype, is_device, label_off, labels, budget, row0, fr, groups))
      return rc;
    res->ms[0] = fr.sniff_ms;
    PosteriorsLaunch pl;
    for (auto& g : groups) {
      if (int rc = posteriors_launch(dec, g, fr, row0, utt_frames, label_off, NL, tc, dtype, dense, pl)) return rc;
      const std::vector<int64_t>& tab_off = pl.tab_off;
      res->launches += pl.launches;
      res->launched[0] += pl.count[0];
      res->launched[1] += pl.count[1];
      // a dense result leaves with its launch: the next one takes the tables over
      for (size_t j = 0; dense && j < g.size(); ++j) {
        const size_t u = (size_t)g[j];
        const size_t cnt = (size_t)(res->gamma_off[u + 1] - res->gamma_off[u]);
        if (cnt && be::d2h(res->gamma.data() + res->gamma_off[u], (const double*)dec->w_ptab.p + tab_off[j], cnt * 8, &err))
          return fail(CTCDEC_ERR_DEVICE, err);
      }
    }
    std::vector<double> pair(2 * n);
    if (be::d2h(pair.data(), dec->w_ascore.p, n * 16, &err)) return fail(CTCDEC_ERR_DEVICE, err);
    for (size_t u = 0; u < n; ++u)
      if (utt_frames[u] > 0) res->logp[u] = pair[2 * u], res->logp_backward[u] = pair[2 * u + 1];
    if (NL && (be::d2h(res->occupancy.data(), dec->w_pocc.p, (size_t)NL * 8, &err) ||
               be::d2h(res->centre.data(), (const double*)dec->w_pocc.p + NL, (size_t)NL * 8, &err)))
      return fail(CTCDEC_ERR_DEVICE, err);
#ifndef CTC_SIM
    res->ms[1] = be::align_kernel_ms(be::K_ROW_LSE);
    res->ms[2] = be::align_kernel_ms(be::K_POSTERIORS);
#endif
  }
  res->ms[3] = ms(t_begin, Clock::now());
  *out = res.release();
  return CTCDEC_OK;
}

int ctcdec_posteriors_scores(const ctcdec_posteriors* p, const double** logp_out, const double** logp_backward_out, int64_t* n_utts_out) {
  if (!p || !logp_out || !logp_backward_out || !n_utts_out) return fail(CTCDEC_ERR_ARG, "no posteriors");
  *logp_out = p->logp.data();
  *logp_backward_out = p->logp_backward.data();
  *n_utts_out = (int64_t)p->logp.size();
  return CTCDEC_OK;
}

int ctcdec_posteriors_tokens(const ctcdec_posteriors* p, const int64_t** tok_off_out, const double** occupancy_out, const double** centre_out,
                             int64_t* n_tokens_out) {
  if (!p || !tok_off_out || !occupancy_out || !centre_out || !n_tokens_out) return fail(CTCDEC_ERR_ARG, "no posteriors");
  *tok_off_out = p->tok_off.data();
  *occupancy_out = p->occupancy.data();
  *centre_out = p->centre.data();
  *n_tokens_out = (int64_t)p->occupancy.size();
  return CTCDEC_OK;
}

int ctcdec_posteriors_gamma(const ctcdec_posteriors* p, const int64_t** gamma_off_out, const int32_t** row_stride_out, const double** gamma_out) {
  if (!p || !gamma_off_out || !row_stride_out || !gamma_out) return fail(CTCDEC_ERR_ARG, "no posteriors");
  *gamma_off_out = p->gamma_off.data();
  *row_stride_out = p->gamma_stride.data();
  *gamma_out = p->dense ? p->gamma.data() : nullptr;
  return CTCDEC_OK;
}

int ctcdec_posteriors_timing(const ctcdec_posteriors* p, double* ms4, int32_t* launches_out, int64_t* launched2) {
  if (!p || !ms4) return fail(CTCDEC_ERR_ARG, "no posteriors");
  for (int k = 0; k < 4; ++k) ms4[k] = p->ms[k];
  if (launches_out) *launches_out = p->launches;
  if (launched2) launched2[0] = p->launched[0], launched2[1] = p->launched[1];
  return CTCDEC_OK;
}

void ctcdec_posteriors_free(ctcdec_posteriors* p) { delete p; }

// ---- transcript gradient ("Transcript gradient") ------------------------------------------------------------------
}  // extern "C"

#ifdef CTC_SIM
namespace {
struct GradSeqCtx {
  enum { KEEP = 1 };  // (ctc_grad_row: the one thread owns every entry, and forms each share in both passes)
  int tid = 0, nt = 1;
  double sum(double v, int) { return v; }
};
template <int DT>
void grad_rows_seq(const std::vector<GradUtt>& utts, int V, int blank, double clip_lo) {
  typedef typename std::conditional<DT == 1, double, float>::type GT;  // (f64 for f64 rows, f32 for every other dtype)
  GradSeqCtx cx;
  for (const GradUtt& u : utts)
    for (int t = 0; t < u.T; ++t) ctc_grad_row<DT, GT>(cx, u, t, V, blank, clip_lo);
}
}  // namespace
#endif

extern "C" {

int ctcdec_gradient_batch(ctcdec_decoder* dec, const void* const* utt_logits, const int32_t* utt_frames, int32_t n_utts, int32_t dtype,
                          int32_t is_device, const int64_t* label_off, const int32_t* labels, void* const* grad_out, int32_t grad_dtype,
                          int64_t table_budget, double* logp_out, double* ms5, int32_t* launches_out, int64_t* launched2) {
  TranscriptCall tc;
  const bool args_ok = dec && n_utts >= 0 && label_off && table_budget >= 0 &&
                       (n_utts == 0 || (utt_logits && utt_frames && grad_out && logp_out));
  const bool grad_ok = grad_dtype == (dtype == CTCDEC_F64 ? CTCDEC_F64 : CTCDEC_F32);
  if (int rc = transcript_open(dec, args_ok, dtype, grad_ok ? "" : "grad_dtype must be f64 for f64 logits and f32 for every other dtype", tc))
    return rc;
  const int V = tc.V;
  const int64_t budget = table_budget ? table_budget : POSTERIORS_TABLE_BUDGET;
  if (int rc = check_posteriors(utt_logits, utt_frames, n_utts, label_off, labels, budget, tc)) return rc;
  for (int32_t u = 0; u < n_utts; ++u)
    if (utt_frames[u] > 0 && !grad_out[u]) return fail(CTCDEC_ERR_ARG, "utterance " + std::to_string(u) + ": no gradient buffer");
  const auto t_begin = Clock::now();
  const size_t n = (size_t)n_utts;
  const int64_t NL = label_off[n];
  const std::vector<int64_t> row0 = row_starts(utt_frames, n);
  const int64_t R = row0[n];
  const size_t gsz = grad_dtype == CTCDEC_F64 ? 8 : 4;
  double tms[5] = {0, 0, 0, 0, 0};
  int32_t launches = 0;
  int64_t launched[2] = {0, 0};
  for (size_t u = 0; u < n; ++u) logp_out[u] = 0.0;  // (no frames and the empty target: the one empty alignment)
  if (R > 0) {
    std::string err;
    AlignFront fr;
    std::vector<std::vector<int32_t>> groups;
    if (int rc = posteriors_front(dec, tc, utt_logits, utt_frames, n_utts, dtype, is_device, label_off, labels, budget, row0, fr, groups))
      return rc;
    tms[0] = fr.sniff_ms;
    // every utterance's occurrence lists: [n][V + 1] offsets into its own part of the [NL] states, which are 2 k + 1 in the
    // order of k under each label
    std::vector<int32_t> occ(n * (size_t)(V + 1) + (size_t)std::max<int64_t>(NL, 1), 0);
    int32_t* const occ_state = occ.data() + n * (size_t)(V + 1);
    std::vector<int32_t> next((size_t)V);
    for (size_t u = 0; u < n; ++u) {
      int32_t* off = occ.data() + u * (size_t)(V + 1);
      const int32_t* lab = labels + label_off[u];
      const int32_t L = (int32_t)(label_off[u + 1] - label_off[u]);
      for (int32_t k = 0; k < L; ++k) ++off[lab[k] + 1];
      for (int v = 0; v < V; ++v) off[v + 1] += off[v], next[(size_t)v] = off[v];
      for (int32_t k = 0; k < L; ++k) occ_state[label_off[u] + next[(size_t)lab[k]]++] = 2 * k + 1;
    }
    if (upload(dec->w_gocc, occ, &err)) return fail(CTCDEC_ERR_DEVICE, err);
    const int32_t* const d_occ_off = (const int32_t*)dec->w_gocc.p;
    const int32_t* const d_occ_state = d_occ_off + n * (size_t)(V + 1);
    if (!is_device) {  // a launch's rows leave through a buffer of the device's own
      int64_t rows = 0;
      for (const auto& g : groups) {
        int64_t r = 0;
        for (int32_t u : g) r += utt_frames[u];
        rows = std::max(rows, r);
      }
      if (dec->w_grad.ensure((size_t)rows * (size_t)V * gsz, &err)) return fail(CTCDEC_ERR_DEVICE, err);
    }
    PosteriorsLaunch pl;
    std::vector<GradUtt> gutts;
    for (auto& g : groups) {
      if (int rc = posteriors_launch(dec, g, fr, row0, utt_frames, label_off, NL, tc, dtype, 1, pl)) return rc;
      launches += pl.launches;
      launched[0] += pl.count[0];
      launched[1] += pl.count[1];
      // the launch's rows, on the same stream, before the next launch takes the tables over
      gutts.clear();
      int64_t rows = 0;
      for (size_t j = 0; j < g.size(); ++j) {
        const size_t u = (size_t)g[j];
        GradUtt a;
        a.x = fr.ptrs[u];
        a.lse = fr.lse + row0[u];
        a.table = (const double*)dec->w_ptab.p + pl.tab_off[j];
        a.occ_off = d_occ_off + u * (size_t)(V + 1);
        a.occ_state = d_occ_state + label_off[u];
        a.grad = is_device ? grad_out[u] : (void*)((char*)dec->w_grad.p + (size_t)rows * (size_t)V * gsz);
        a.row_begin = rows;
        a.T = utt_frames[u];
        a.L = (int32_t)(label_off[u + 1] - label_off[u]);
        a.is_prob = fr.is_prob[u] ? 1 : 0;
        a.pad = 0;
        gutts.push_back(a);
        rows += utt_frames[u];
      }
#ifdef CTC_SIM  // (the kernel's body, row by row)
      for_dtype(dtype, [&](auto dt) { grad_rows_seq<decltype(dt)::value>(gutts, V, tc.blank, tc.clip_lo); });
#else
      if (upload(dec->w_gutts, gutts, &err)) return fail(CTCDEC_ERR_DEVICE, err);
      be::GradRowsArgs ga;
      ga.utts = (const GradUtt*)dec->w_gutts.p;
      ga.n_utts = (int32_t)gutts.size();
      ga.n_labels = V;
      ga.n_rows = rows;
      ga.dtype = dtype;
      ga.grad_dtype = grad_dtype;
      ga.blank = tc.blank;
      ga.pad = 0;
      ga.clip_lo = tc.clip_lo;
      if (be::launch_ctc_grad_rows(ga, &err)) return fail(CTCDEC_ERR_DEVICE, err);
#endif
      ++launches;
      for (size_t j = 0; !is_device && j < g.size(); ++j) {
        const size_t u = (size_t)g[j];
        const size_t bytes = (size_t)utt_frames[u] * (size_t)V * gsz;
        if (be::d2h(grad_out[u], gutts[j].grad, bytes, &err)) return fail(CTCDEC_ERR_DEVICE, err);
      }
    }
    std::vector<double> pair(2 * n);
    if (be::d2h(pair.data(), dec->w_ascore.p, n * 16, &err)) return fail(CTCDEC_ERR_DEVICE, err);  // (waits for the last launch)
    for (size_t u = 0; u < n; ++u)
      if (utt_frames[u] > 0) logp_out[u] = pair[2 * u];
#ifndef CTC_SIM
    tms[1] = be::align_kernel_ms(be::K_ROW_LSE);
    tms[2] = be::align_kernel_ms(be::K_POSTERIORS);
    tms[3] = be::align_kernel_ms(be::K_GRAD_ROWS);
#endif
  }
  tms[4] = ms(t_begin, Clock::now());
  if (ms5)
    for (int k = 0; k < 5; ++k) ms5[k] = tms[k];
  if (launches_out) *launches_out = launches;
  if (launched2) launched2[0] = launched[0], launched2[1] = launched[1];
  return CTCDEC_OK;
}

// ---- phrase search ("Phrase search") ---------------------------------------------------------------------------------
}  // extern "C"

struct ctcdec_search {
  std::vector<int64_t> hit_off, trace_off;
  std::vector<int32_t> start, end, end_start;
  std::vector<double> logp, end_logp;
  bool has_trace = false;
  int32_t launches = 0;
  int64_t launched[2] = {0, 0};
  double ms[4] = {0, 0, 0, 0};
};

// A launched phrase's trace: a float64 end_logp and an int32 end_start per frame. The traces of one launch come under the
// budget of the alignment's back-pointer tables (ALIGN_BP_BUDGET) when the caller names none.
static const int64_t FIND_TRACE_BYTES = 12;

#ifdef CTC_SIM
namespace {
// (ctc_find_phrase: the one thread owns every group and is the whole "wavefront" of the selection)
struct FindSeqCtx {
  enum { GROUPS = FORWARD_MAX_GROUPS };
  int tid = 0, nt = 1;
  int32_t hs[FIND_MAX_HITS], he[FIND_MAX_HITS];
  void sync() {}
  bool same_wave(int) const { return true; }
  void publish() const {}
  int lane() const { return 0; }
  int lanes() const { return 1; }
  bool any(bool b) const { return b; }
  void best(double&, int&, int&) const {}
  void put(int j, int32_t s, int32_t e) { hs[j] = s, he[j] = e; }
  void get(int j, int32_t* s, int32_t* e) const { *s = hs[j], *e = he[j]; }
};
static_assert(FORWARD_MAX_GROUPS >= find_chunks(ALIGN_MAX_LABELS), "a group per four states of the longest phrase");
}  // namespace
#endif

extern "C" {

int ctcdec_find_batch(ctcdec_decoder* dec, const void* const* utt_logits, const int32_t* utt_frames, int32_t n_utts, int32_t dtype,
                      int32_t is_device, const int64_t* hyp_off, const int64_t* label_off, const int32_t* labels, int32_t max_hits,
                      double min_logp, int32_t want_trace, int32_t kernel, int64_t trace_budget, ctcdec_search** out) {
  TranscriptCall tc;
  const bool args_ok = dec && out && n_utts >= 0 && label_off && hyp_off && trace_budget >= 0 && (n_utts == 0 || (utt_logits && utt_frames));
  std::string bad_option = bad_kernel(kernel);
  if (bad_option.empty() && (max_hits < 1 || max_hits > FIND_MAX_HITS)) bad_option = "max_hits must be in 1 .. " + std::to_string(FIND_MAX_HITS);
  if (bad_option.empty() && min_logp != min_logp) bad_option = "min_logp is not a number";
  if (int rc = transcript_open(dec, args_ok, dtype, bad_option, tc)) return rc;
  std::vector<int32_t> need;
  if (int rc = check_scores(utt_logits, utt_frames, n_utts, labels, label_off, hyp_off, tc, need, "phrase")) return rc;
  const size_t n = (size_t)n_utts;
  const int64_t NH = hyp_off[n];
  const int64_t budget = trace_budget ? trace_budget : ALIGN_BP_BUDGET;
  for (int32_t u = 0; u < n_utts; ++u)
    for (int64_t h = hyp_off[u]; h < hyp_off[u + 1]; ++h) {
      const std::string who = "utterance " + std::to_string(u) + ", phrase " + std::to_string(h - hyp_off[u]);
      if (label_off[h + 1] == label_off[h]) return fail(CTCDEC_ERR_ARG, who + ": an empty phrase occurs everywhere and nowhere");
      if (utt_frames[u] >= need[(size_t)h] && FIND_TRACE_BYTES * utt_frames[u] > budget)
        return fail(CTCDEC_ERR_LIMIT, who + ": a trace of " + std::to_string(FIND_TRACE_BYTES * utt_frames[u]) +
                                          " bytes, above the budget of " + std::to_string(budget) + " bytes for one launch");
    }
  const auto t_begin = Clock::now();
  std::unique_ptr<ctcdec_search> res(new ctcdec_search());
  res->has_trace = want_trace != 0;
  // A phrase with fewer frames than labels plus adjacent equal labels occurs nowhere: no hits, decided here. Everything else
  // goes to a kernel: the wave kernel up to its limit (unless the group kernel is forced), the group kernel above it.
  const int32_t wave_max = kernel == 2 ? -1 : FIND_WAVE_MAX_LABELS;
  const Routed routed = route_items(hyp_off, label_off, utt_frames, n_utts, need, wave_max);  // (its launches sort for themselves)
  const std::vector<int32_t>& utt_of = routed.utt_of;
  res->trace_off.assign((size_t)NH + 1, 0);
  for (int64_t h = 0; h < NH; ++h) res->trace_off[(size_t)h + 1] = res->trace_off[(size_t)h] + (want_trace ? utt_frames[utt_of[(size_t)h]] : 0);
  if (want_trace) {  // (a phrase that is not launched ends nowhere)
    res->end_logp.assign((size_t)res->trace_off[(size_t)NH], align_neg_inf());
    res->end_start.assign((size_t)res->trace_off[(size_t)NH], -1);
  }
  std::vector<int32_t> n_hits((size_t)NH, 0), h_start, h_end;
  std::vector<double> h_logp;
  const size_t K = (size_t)max_hits;
  if (routed.any()) {
    const std::vector<int32_t>& use_frames = routed.use_frames;
    const std::vector<int64_t> row0 = row_starts(use_frames.data(), n);
    const int64_t NL = label_off[NH];
    std::string err;
    AlignFront fr;
    if (int rc = align_front(dec, utt_logits, use_frames.data(), n_utts, dtype, is_device, tc.V, row0, fr)) return rc;
    res->ms[0] = fr.sniff_ms;
    // the call's hits: per phrase max_hits scores, then as many starts and ends, then the counts
    const size_t hits_bytes = (size_t)NH * K * 16 + (size_t)NH * 4;
    if (dec->w_alab.ensure((size_t)NL * 4, &err) || dec->w_fhits.ensure(hits_bytes, &err)) return fail(CTCDEC_ERR_DEVICE, err);
    if (be::h2d(dec->w_alab.p, labels, (size_t)NL * 4, &err) || be::zero(dec->w_fhits.p, hits_bytes, &err))
      return fail(CTCDEC_ERR_DEVICE, err);
    double* const d_logp = (double*)dec->w_fhits.p;
    int32_t* const d_start = (int32_t*)(d_logp + (size_t)NH * K);
    int32_t* const d_end = d_start + (size_t)NH * K;
    int32_t* const d_count = d_end + (size_t)NH * K;
    // launches: the launched phrases in input order until their traces fill the budget
    std::vector<std::vector<int32_t>> groups;
    const auto bytes_of = [&](int32_t h) {
      const int64_t T = utt_frames[utt_of[(size_t)h]];
      return T >= need[(size_t)h] ? FIND_TRACE_BYTES * T : 0;
    };
    const int64_t most = budget_groups((int32_t)NH, bytes_of, budget, groups);
    if (dec->w_ftrace.ensure((size_t)most, &err)) return fail(CTCDEC_ERR_DEVICE, err);
    std::vector<FindPhrase> phrases;
    std::vector<double> t_logp;
    std::vector<int32_t> t_start;
    for (auto& g : groups) {
      // inside a launch the wave kernel's phrases come before the group kernel's, longest utterance first in each; the scores
      // of the launch's traces lie before its start frames, each in that order
      std::stable_sort(g.begin(), g.end(), [&](int32_t a, int32_t b) {
        const bool wa = label_off[a + 1] - label_off[a] <= wave_max, wb = label_off[b + 1] - label_off[b] <= wave_max;
        return wa != wb ? wa : utt_frames[utt_of[(size_t)a]] > utt_frames[utt_of[(size_t)b]];
      });
      int64_t frames = 0;
      for (int32_t h : g) frames += utt_frames[utt_of[(size_t)h]];
      double* const tr_logp = (double*)dec->w_ftrace.p;
      int32_t* const tr_start = (int32_t*)(tr_logp + frames);
      phrases.clear();
      int32_t count[2] = {0, 0}, max_chunks[2] = {1, 1};
      int64_t off = 0;
      for (int32_t h : g) {
        const int32_t u = utt_of[(size_t)h];
        FindPhrase a;
        a.x = fr.ptrs[(size_t)u];
        a.lse = fr.lse + row0[(size_t)u];
        a.lab = (const int32_t*)dec->w_alab.p + label_off[h];
        a.end_logp = tr_logp + off;
        a.end_start = tr_start + off;
        a.hit_logp = d_logp + (size_t)h * K;
        a.hit_start = d_start + (size_t)h * K;
        a.hit_end = d_end + (size_t)h * K;
        a.n_hits = d_count + h;
        a.T = utt_frames[u];
        a.L = (int32_t)(label_off[h + 1] - label_off[h]);
        a.is_prob = fr.is_prob[(size_t)u] ? 1 : 0;
        a.pad = 0;
        phrases.push_back(a);
        off += a.T;
        const int w = a.L <= wave_max ? 0 : 1;
        max_chunks[w] = std::max(max_chunks[w], find_chunks(a.L));
        ++count[w];
      }
#ifdef CTC_SIM  // (both kernels are the one body here: a single thread owns every group)
      std::vector<double> col((size_t)3 * (size_t)std::max(max_chunks[0], max_chunks[1]));
      FindSeqCtx cx;
      for (const FindPhrase& a : phrases)
        for_dtype(dtype, [&](auto dt) {
          ctc_find_phrase<decltype(dt)::value>(cx, a, tc.V, tc.blank, tc.clip_lo, max_hits, min_logp, col.data());
        });
      for (int w = 0; w < 2; ++w) res->launches += count[w] ? 1 : 0;
#else
      if (upload(dec->w_fphr, phrases, &err)) return fail(CTCDEC_ERR_DEVICE, err);
      for (int w = 0; w < 2; ++w) {
        if (!count[w]) continue;
        be::FindArgs fa;
        fa.phrases = (const FindPhrase*)dec->w_fphr.p + (w ? count[0] : 0);
        fa.n_phrases = count[w];
        fa.n_labels = tc.V;
        fa.dtype = dtype;
        fa.blank = tc.blank;
        fa.max_chunks = max_chunks[w];
        fa.max_hits = max_hits;
        fa.clip_lo = tc.clip_lo;
        fa.min_logp = min_logp;
        if (be::launch_ctc_find(fa, w == 0, &err)) return fail(CTCDEC_ERR_DEVICE, err);
        ++res->launches;
      }
#endif
      res->launched[0] += count[0];
      res->launched[1] += count[1];
      if (want_trace) {  // a launch's traces leave with it: the next one takes the workspace over
        t_logp.resize((size_t)frames);
        t_start.resize((size_t)frames);
        if (be::d2h(t_logp.data(), tr_logp, (size_t)frames * 8, &err) || be::d2h(t_start.data(), tr_start, (size_t)frames * 4, &err))
          return fail(CTCDEC_ERR_DEVICE, err);
        off = 0;
        for (int32_t h : g) {
          const size_t T = (size_t)utt_frames[utt_of[(size_t)h]];
          std::copy(t_logp.begin() + off, t_logp.begin() + off + (int64_t)T, res->end_logp.begin() + res->trace_off[(size_t)h]);
          std::copy(t_start.begin() + off, t_start.begin() + off + (int64_t)T, res->end_start.begin() + res->trace_off[(size_t)h]);
          off += (int64_t)T;
        }
      }
    }
    h_logp.resize((size_t)NH * K);
    h_start.resize((size_t)NH * K);
    h_end.resize((size_t)NH * K);
    if (be::d2h(h_logp.data(), d_logp, (size_t)NH * K * 8, &err) || be::d2h(h_start.data(), d_start, (size_t)NH * K * 4, &err) ||
        be::d2h(h_end.data(), d_end, (size_t)NH * K * 4, &err) || be::d2h(n_hits.data(), d_count, (size_t)NH * 4, &err))
      return fail(CTCDEC_ERR_DEVICE, err);
#ifndef CTC_SIM
    res->ms[1] = be::align_kernel_ms(be::K_ROW_LSE);
    res->ms[2] = be::align_kernel_ms(be::K_FIND);
#endif
  }
  res->hit_off.assign((size_t)NH + 1, 0);
  for (size_t h = 0; h < (size_t)NH; ++h) {
    if (n_hits[h] < 0 || n_hits[h] > max_hits) return fail(CTCDEC_ERR_DEVICE, "ctc_find returned a hit count outside 0 .. max_hits");
    res->hit_off[h + 1] = res->hit_off[h] + n_hits[h];
    for (size_t j = 0; j < (size_t)n_hits[h]; ++j) {
      res->start.push_back(h_start[h * K + j]);
      res->end.push_back(h_end[h * K + j]);
      res->logp.push_back(h_logp[h * K + j]);
    }
  }
  res->ms[3] = ms(t_begin, Clock::now());
  *out = res.release();
  return CTCDEC_OK;
}

int ctcdec_search_hits(const ctcdec_search* s, const int64_t** hit_off_out, const int32_t** start_out, const int32_t** end_out,
                       const double** logp_out, int64_t* n_phrases_out) {
  if (!s || !hit_off_out || !start_out || !end_out || !logp_out || !n_phrases_out) return fail(CTCDEC_ERR_ARG, "no search");
  *hit_off_out = s->hit_off.data();
  *start_out = s->start.data();
  *end_out = s->end.data();
  *logp_out = s->logp.data();
  *n_phrases_out = (int64_t)s->hit_off.size() - 1;
  return CTCDEC_OK;
}

int ctcdec_search_trace(const ctcdec_search* s, const int64_t** trace_off_out, const double** end_logp_out, const int32_t** end_start_out) {
  if (!s || !trace_off_out || !end_logp_out || !end_start_out) return fail(CTCDEC_ERR_ARG, "no search");
  *trace_off_out = s->trace_off.data();
  *end_logp_out = s->has_trace ? s->end_logp.data() : nullptr;
  *end_start_out = s->has_trace ? s->end_start.data() : nullptr;
  return CTCDEC_OK;
}

int ctcdec_search_timing(const ctcdec_search* s, double* ms4, int32_t* launches_out, int64_t* launched2) {
  if (!s || !ms4) return fail(CTCDEC_ERR_ARG, "no search");
  for (int k = 0; k < 4; ++k) ms4[k] = s->ms[k];
  if (launches_out) *launches_out = s->launches;
  if (launched2) launched2[0] = s->launched[0], launched2[1] = s->launched[1];
  return CTCDEC_OK;
}

void ctcdec_search_free(ctcdec_search* s) { delete s; }
}  // extern "C"
