// ctc_align.h -- what is computed from an utterance's frames and a known label sequence ("Forced alignment" to
// "Alignment with gaps"), over the states blank / label / blank / ... One body each for the HIP kernels (ctc_align_hip.hip)
// and for the CPU simulator build, whose "device" memory is host memory (api_transcript.cpp under CTC_SIM runs them with a one-thread
// context). The bodies:
//   row_lse_seq, row_lse_max_seq   a row's fp64 log-sum-exp (and maximum): the simulator's; the kernels fold by lanes
//   ctc_viterbi_utt                the best path, its columns in LDS            (kernel ctc_viterbi)
//   ctc_viterbi_long_utt           the best path, its columns in device memory, its frames in segments  (ctc_viterbi_long)
//   ctc_forward_hyp / _wave_hyp    the sum over all paths                       (ctc_forward / ctc_forward_wave)
//   ctc_posteriors_utt             the forward-backward                         (ctc_posteriors)
//   ctc_grad_row                   the gradient of the likelihood, row by row   (ctc_grad_rows)
//   ctc_find_phrase / _wave_phrase a phrase's occurrences, free start and end   (ctc_find / ctc_find_wave)
//   ctc_viterbi_gaps_utt           the best path of a target with gaps          (ctc_viterbi_gaps)
//   row_argmax_seq                 a row's most probable label: the simulator's; the kernels fold by lanes
//   greedy_collapse_utt            runs of frame labels to tokens               (greedy_collapse)
//   ctc_forward_hyp / _wave_hyp <ENDS>  the forward pass that also stores a prefix' end states  (ctc_forward_ends / ctc_forward_wave_ends)
//   ctc_prefix_extend_tile, ctc_prefix_finish_col   every label's prefix score from them  (ctc_prefix_extend, ctc_prefix_finish)
//   ctc_prefix_advance_child       a child prefix' end states from its parent's  (ctc_prefix_advance)
// The shared pieces, and who uses them:
//   viterbi_backtrace                                    ctc_viterbi, ctc_viterbi_gaps
//   viterbi_backtrace_span (a segment of it)             ctc_viterbi_long
//   fold_token_logp                                      ctc_viterbi, ctc_viterbi_gaps, ctc_viterbi_long
//   group_setup, EntrySource, FrameEntries               ctc_find, ctc_find_wave, ctc_viterbi_gaps
//   thread_setup                                         ctc_find, ctc_viterbi_gaps
// ctc_forward_hyp, ctc_forward_wave_hyp and ctc_posteriors_utt keep their loops in raw variables: over FrameEntries
// ctc_forward took 8 to 13 % and ctc_posteriors 2 % longer on batches of 64 utterances (profiles/align_refactor_check.txt).
//   find_trace, find_select                              ctc_find, ctc_find_wave
//   for_dtype (host)                                     the launchers and the simulator's calls
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "common.h"
#include "np_sum.h"
#include "token_logp.h"

namespace ctc {

constexpr int32_t ALIGN_MAX_LABELS = 2047;  // 4095 states: two fp64 score columns of 4096 entries are the 64 KB of LDS a workgroup may use
constexpr int32_t ALIGN_THREADS = 256;
constexpr int32_t ALIGN_LSE_BLOCK = 16;     // values a lane folds under one rescale of its running sum

// One utterance of a ctc_viterbi launch. The host validates every field before a launch: the labels are in [0, V) and not the
// blank, T >= L + (adjacent equal labels) >= 1, and every array is as long as its comment says.
struct AlignUtt {
  const void* x;       // [T, V] logits or probabilities, of the launch's dtype
  const double* lse;   // [T] log-sum-exp of each row (not read when is_prob)
  const int32_t* lab;  // [L] target labels
  uint8_t* bp;         // [T * align_chunks(L)] back-pointers, four 2-bit entries per byte
  int32_t* path;       // [T] out: the label taken at each frame, the blank id for blanks
  int32_t* tok_start;  // [L] out: first frame of each target label
  int32_t* tok_end;    // [L] out: one past its last frame
  double* tok_logp;    // [L] out (fold != 0): the fold of the label's log-probability over [tok_start, tok_end)
  double* score;       // [1] out: the sum of the log-probabilities along `path`
  int32_t T, L, is_prob, pad;
};

CTC_HD int32_t align_chunks(int32_t L) { return (2 * L + 1 + 3) >> 2; }  // groups of four states

CTC_HD double align_neg_inf() { return -HUGE_VAL; }

// x[i] of a matrix of dtype code 0 f32 / 1 f64 / 2 f16 / 3 bf16, widened (exactly) to double
CTC_HD double align_load(const void* x, int dtype, size_t i) {
  if (dtype == 0) return (double)((const float*)x)[i];
  if (dtype == 1) return ((const double*)x)[i];
  const uint16_t h = ((const uint16_t*)x)[i];
  return (double)(dtype == 2 ? f16_bits_to_f32(h) : bf16_bits_to_f32(h));
}

// The log-probability the alignment sees for one entry: log(clip(p, 1e-15, 1)) of a probability-like utterance, else
// clip(x - lse, ln 1e-15, 0). A NaN takes the floor, so that every score stays ordered.
// (of_value: of an entry loaded earlier -- the forward kernels ask for a frame's entries one frame ahead of their use)
CTC_HD double align_emit_of_value(double v, double lse, bool is_prob, double clip_lo) {
  if (is_prob) return log(!(v >= 1e-15) ? 1e-15 : (v > 1.0 ? 1.0 : v));
  const double y = v - lse;
  return !(y >= clip_lo) ? clip_lo : (y > 0.0 ? 0.0 : y);
}
CTC_HD double align_emit(const void* x, int dtype, size_t i, double lse, bool is_prob, double clip_lo) {
  return align_emit_of_value(align_load(x, dtype, i), lse, is_prob, clip_lo);
}

// ---- row_lse: running maximum m and sum of exp(x - m) --------------------------------------------------------------------
struct LseAcc {
  double m, s;
};
CTC_HD LseAcc lse_empty() { return LseAcc{align_neg_inf(), 0.0}; }
// ALIGN_LSE_BLOCK values at once (unused slots hold -inf): one exp for the rescale, one per value
CTC_HD void lse_push_block(LseAcc& a, const double* v) {
  double bm = align_neg_inf();
  CTC_UNROLL
  for (int i = 0; i < ALIGN_LSE_BLOCK; ++i) bm = v[i] > bm ? v[i] : bm;
  if (bm > a.m) {
    a.s *= exp(a.m - bm);  // (a.m = -inf: s is 0 and stays 0)
    a.m = bm;
  }
  if (!(a.m > align_neg_inf())) return;
  CTC_UNROLL
  for (int i = 0; i < ALIGN_LSE_BLOCK; ++i)
    if (v[i] > align_neg_inf()) a.s += exp(v[i] - a.m);
}
CTC_HD void lse_push(LseAcc& a, double v) {
  if (v > a.m) {
    a.s = a.s * exp(a.m - v) + 1.0;
    a.m = v;
  } else if (v > align_neg_inf()) {
    a.s += exp(v - a.m);
  }
}
CTC_HD LseAcc lse_merge(const LseAcc& a, const LseAcc& b) {
  const double m = a.m > b.m ? a.m : b.m;
  if (!(m > align_neg_inf())) return LseAcc{m, 0.0};
  return LseAcc{m, a.s * exp(a.m - m) + b.s * exp(b.m - m)};
}
CTC_HD double lse_value(const LseAcc& a) { return a.m + log(a.s); }

// One row, one thread (the simulator; the kernel spreads the same blocks over the lanes of a wave)
CTC_HD LseAcc row_fold_seq(const void* x, int dtype, size_t row0, int V) {
  LseAcc a = lse_empty();
  double v[ALIGN_LSE_BLOCK];
  for (int b = 0; b < V; b += ALIGN_LSE_BLOCK) {
    for (int i = 0; i < ALIGN_LSE_BLOCK; ++i) v[i] = b + i < V ? align_load(x, dtype, row0 + (size_t)(b + i)) : align_neg_inf();
    lse_push_block(a, v);
  }
  return a;
}
CTC_HD double row_lse_seq(const void* x, int dtype, size_t row0, int V) { return lse_value(row_fold_seq(x, dtype, row0, V)); }

// ---- ctc_viterbi -------------------------------------------------------------------------------------------------------------
// State s of the 2L+1: even = a blank, odd = target label s >> 1. A thread owns groups of four consecutive states (blank,
// label 2c, blank, label 2c + 1), reads the previous column of scores from `col`, writes the current one and one byte of four
// back-pointers (0 stay, 1 step, 2 skip). Equal scores prefer stay, then step, then skip. Frame t only works on the groups
// that hold a state reachable from the start (s <= 2t + 1) and from the end (s >= S - 2 - 2(T - 1 - t)); what lies below the
// window of the previous frame reads as unreachable. `col`: 2 * 4 * align_chunks(L) doubles, shared by the threads of cx.
// cx: tid, nt, sync().

// The back-trace, by one thread: from state s of the last frame along the 2-bit back-pointers (four to a byte, nch bytes a
// frame) to frame 0. Writes the path -- a label state its label, the even state 2j slot_value(j): the blank, or -1 for a gap
// slot of ctc_viterbi_gaps -- and the span of every label.
template <class SlotValue>
CTC_HD void viterbi_backtrace(int s, int T, int nch, const uint8_t* bp, const int32_t* lab, int32_t* path, int32_t* tok_start,
                              int32_t* tok_end, SlotValue slot_value) {
  int open = -1;
  for (int t = T - 1; t >= 0; --t) {
    if (s & 1) {
      const int k = s >> 1;
      if (k != open) tok_end[k] = t + 1, open = k;
      tok_start[k] = t;
      path[t] = lab[k];
    } else {
      path[t] = slot_value(s >> 1);
    }
    if (t > 0) {
      const unsigned b = (bp[(size_t)t * (size_t)nch + (size_t)(s >> 2)] >> (2 * (s & 3))) & 3u;
      s -= (int)b;
      if (s < 0) s = 0;
    }
  }
}
// viterbi_backtrace_span: the frames t_hi down to t_lo of it, from state s of frame t_hi; frame t's back-pointers are row
// t - row0 of bp. Leaves in s the state of frame t_lo - 1 (of frame 0 when t_lo is 0) and in `open` the label whose span is
// still open -- a span may go on below t_lo: the next span, over the frames below, takes both over (ctc_viterbi_long).
// viterbi_backtrace is this over (T - 1, 0, row 0) with nothing open; written as that call, ctc_viterbi and ctc_viterbi_gaps
// compile to other instructions (tools/kernel_asm_diff.py), so it keeps its own loop.
template <class SlotValue>
CTC_HD void viterbi_backtrace_span(int& s, int& open, int t_hi, int t_lo, int row0, int nch, const uint8_t* bp, const int32_t* lab,
                                   int32_t* path, int32_t* tok_start, int32_t* tok_end, SlotValue slot_value) {
  for (int t = t_hi; t >= t_lo; --t) {
    if (s & 1) {
      const int k = s >> 1;
      if (k != open) tok_end[k] = t + 1, open = k;
      tok_start[k] = t;
      path[t] = lab[k];
    } else {
      path[t] = slot_value(s >> 1);
    }
    if (t > 0) {
      const unsigned b = (bp[(size_t)(t - row0) * (size_t)nch + (size_t)(s >> 2)] >> (2 * (s & 3))) & 3u;
      s -= (int)b;
      if (s < 0) s = 0;
    }
  }
}

// The confidence fold, a thread per label: the mean, minimum or maximum of the label's log-probability over its span
template <class Ctx>
CTC_HD void fold_token_logp(Ctx& cx, const void* x, int dtype, const double* lse, const int32_t* lab, const int32_t* tok_start,
                            const int32_t* tok_end, double* tok_logp, int T, int L, int V, bool is_prob, int fold, double clip_lo) {
  for (int k = cx.tid; k < L; k += cx.nt) {
    int t0 = tok_start[k], t1 = tok_end[k];
    t0 = t0 < 0 ? 0 : t0;
    t1 = t1 > T ? T : t1;
    const size_t lb = (size_t)lab[k];
    double acc = 0.0;
    for (int t = t0; t < t1; ++t) {
      const double lp = align_emit(x, dtype, (size_t)t * (size_t)V + lb, is_prob ? 0.0 : lse[t], is_prob, clip_lo);
      if (fold == LOGP_MEAN) acc += lp;
      else if (fold == LOGP_MIN) acc = (t == t0 || lp < acc) ? lp : acc;
      else acc = (t == t0 || lp > acc) ? lp : acc;
    }
    tok_logp[k] = fold == LOGP_MEAN ? acc / (double)(t1 - t0) : acc;
  }
}

template <class Ctx>
CTC_HD void ctc_viterbi_utt(Ctx& cx, const AlignUtt& u, int V, int dtype, int blank, int fold, double clip_lo, double* col) {
  const int T = u.T, L = u.L;
  if (T <= 0) return;
  const int S = 2 * L + 1, nch = align_chunks(L);
  const double NEG = align_neg_inf();
  const bool is_prob = u.is_prob != 0;
  double* c0 = col;
  double* c1 = col + 4 * nch;
  for (int i = cx.tid; i < 8 * nch; i += cx.nt) col[i] = NEG;
  cx.sync();
  if (cx.tid == 0) {
    const double lse0 = is_prob ? 0.0 : u.lse[0];
    c0[0] = align_emit(u.x, dtype, (size_t)blank, lse0, is_prob, clip_lo);
    if (L > 0) c0[1] = align_emit(u.x, dtype, (size_t)u.lab[0], lse0, is_prob, clip_lo);
  }
  cx.sync();
  int prev_lo4 = 0;  // first state of the previous frame's window, rounded down to its group
  for (int t = 1; t < T; ++t) {
    const double* prev = (t & 1) ? c0 : c1;
    double* cur = (t & 1) ? c1 : c0;
    const int lo = S - 2 - 2 * (T - 1 - t), hi = 2 * t + 1;
    const int clo = lo > 0 ? lo >> 2 : 0, chi = (hi < S - 1 ? hi : S - 1) >> 2;
    const double lse_t = is_prob ? 0.0 : u.lse[t];
    const size_t row = (size_t)t * (size_t)V;
    const double e_blank = align_emit(u.x, dtype, row + (size_t)blank, lse_t, is_prob, clip_lo);
    for (int c = clo + cx.tid; c <= chi; c += cx.nt) {
      const int s0 = 4 * c, k0 = 2 * c, k1 = 2 * c + 1;
      const int l0 = k0 < L ? u.lab[k0] : -1, l1 = k1 < L ? u.lab[k1] : -1;
      const int lm1 = k0 > 0 && k0 <= L ? u.lab[k0 - 1] : -1;
      const double pm1 = s0 - 1 >= prev_lo4 ? prev[s0 - 1] : NEG;
      const double p0 = prev[s0], p1 = prev[s0 + 1], p2 = prev[s0 + 2], p3 = prev[s0 + 3];
      // blank s0: stay / step
      double b0 = p0;
      unsigned bp = 0;
      if (pm1 > b0) b0 = pm1, bp = 1u;
      cur[s0] = b0 + e_blank;
      // label k0: stay / step / skip over the blank when the label before differs
      double b1 = NEG, b2 = NEG, b3 = NEG;
      if (l0 >= 0) {
        unsigned q = 0;
        b1 = p1;
        if (p0 > b1) b1 = p0, q = 1u;
        if (lm1 >= 0 && lm1 != l0 && pm1 > b1) b1 = pm1, q = 2u;
        bp |= q << 2;
        b1 += align_emit(u.x, dtype, row + (size_t)l0, lse_t, is_prob, clip_lo);
      }
      if (s0 + 2 < S) {
        unsigned q = 0;
        b2 = p2;
        if (p1 > b2) b2 = p1, q = 1u;
        bp |= q << 4;
        b2 += e_blank;
      }
      if (l1 >= 0) {
        unsigned q = 0;
        b3 = p3;
        if (p2 > b3) b3 = p2, q = 1u;
        if (l1 != l0 && p1 > b3) b3 = p1, q = 2u;
        bp |= q << 6;
        b3 += align_emit(u.x, dtype, row + (size_t)l1, lse_t, is_prob, clip_lo);
      }
      cur[s0 + 1] = b1;
      cur[s0 + 2] = b2;
      cur[s0 + 3] = b3;
      u.bp[(size_t)t * (size_t)nch + (size_t)c] = (uint8_t)bp;
    }
    prev_lo4 = 4 * clo;
    cx.sync();  // the one barrier of a frame: the columns swap roles
  }
  // back-trace: one thread. The last label is preferred over the trailing blank.
  if (cx.tid == 0) {
    const double* fin = ((T - 1) & 1) ? c1 : c0;
    int s = (L > 0 && fin[S - 2] >= fin[S - 1]) ? S - 2 : S - 1;
    *u.score = fin[s];
    viterbi_backtrace(s, T, nch, u.bp, u.lab, u.path, u.tok_start, u.tok_end, [&](int) { return blank; });
  }
  if (!fold) return;
  cx.sync();  // (the spans thread 0 wrote are read by every thread)
  fold_token_logp(cx, u.x, dtype, u.lse, u.lab, u.tok_start, u.tok_end, u.tok_logp, T, L, V, is_prob, fold, clip_lo);
}

// ---- ctc_viterbi_long ---------------------------------------------------------------------------------------------------------
// ctc_viterbi's best path for targets whose columns do not fit LDS and whose back-pointer table does not fit memory
// ("Forced alignment of long transcripts"): the same states, window, operands, order of operations and tie rules,
// so the same bits. Both score columns live in device memory. The frames 1 .. T - 1 are cut into n = ceil((T - 1) / K)
// segments; segment j takes the frames j K + 1 .. min((j + 1) K, T - 1) and starts from the column of frame j K.
//   n == 1: one pass that writes the whole table, then the back-trace -- ctc_viterbi's steps.
//   n > 1:  a pass without back-pointers that copies the column of every frame j K into a checkpoint and ends with the score
//           and the end state; then, from the last segment to the first: the checkpoint restored, the segment's frames once
//           more into a table of K rows, and that segment back-traced from the state the segment above handed down.
constexpr int32_t ALIGN_LONG_MAX_LABELS = 1048575;  // S = 2 L + 1 < 2^21: every index formed from S stays far inside int32
constexpr int32_t ALIGN_LONG_THREADS = 1024;

// One utterance of a ctc_viterbi_long launch, validated by the host as an AlignUtt is. col, ckpt and bp are the utterance's
// own: no other workgroup reads or writes them.
struct AlignLongUtt {
  const void* x;       // [T, V] logits or probabilities, of the launch's dtype
  const double* lse;   // [T] log-sum-exp of each row (not read when is_prob)
  const int32_t* lab;  // [L] target labels
  double* col;         // [2 * 4 * align_chunks(L)] the two score columns
  double* ckpt;        // [n * 4 * align_chunks(L)] (n > 1) the column each segment starts from
  uint8_t* bp;         // [min(K, T - 1) * align_chunks(L)] one segment's back-pointers, four 2-bit entries per byte
  int32_t* path;       // [T] out
  int32_t* tok_start;  // [L] out
  int32_t* tok_end;    // [L] out
  double* tok_logp;    // [L] out (fold != 0)
  double* score;       // [1] out: the last column's value at the end state
  int32_t T, L, is_prob, K;  // 1 <= K <= T: the frames of a segment
};

CTC_HD int32_t align_long_segments(int32_t T, int32_t K) { return T > 1 ? (T - 2) / K + 1 : 0; }  // ceil((T - 1) / K)
CTC_HD int32_t align_long_segment_end(int32_t T, int32_t K, int32_t f) { return T - 1 - f > K ? f + K : T - 1; }

// The frames f + 1 .. e of the recursion, the column of frame f in place (an even frame's in the first column) and the other
// column -inf above frame f's window. BP: frame t's back-pointers go to row t - f - 1 of bp. The loop and the four-state
// update are ctc_viterbi_utt's, a second copy: that body indexes LDS and one table of T rows, this one device memory and a
// table that starts anew with every segment, and shared code would have to leave ctc_viterbi's instructions as they are.
// The window's bounds are formed without 2 * t or 2 * (T - 1 - t), which leave int32 above 2^30 frames: the same values.
template <bool BP, class Ctx>
CTC_HD void viterbi_long_frames(Ctx& cx, const AlignLongUtt& u, int V, int dtype, int blank, double clip_lo, int f, int e, uint8_t* bp) {
  const int T = u.T, L = u.L;
  const int S = 2 * L + 1, nch = align_chunks(L);
  const double NEG = align_neg_inf();
  const bool is_prob = u.is_prob != 0;
  double* c0 = u.col;
  double* c1 = u.col + 4 * nch;
  // first state of frame f's window, rounded down to its group (before frame 1: 0, as ctc_viterbi_utt starts)
  int prev_lo4 = f > 0 && T - 1 - f < L ? 4 * ((2 * (L - (T - 1 - f)) - 1) >> 2) : 0;
  for (int t = f + 1; t <= e; ++t) {
    const double* prev = (t & 1) ? c0 : c1;
    double* cur = (t & 1) ? c1 : c0;
    const int rest = T - 1 - t;  // lo = S - 2 - 2 * rest, hi = 2 * t + 1
    const int clo = rest < L ? (2 * (L - rest) - 1) >> 2 : 0, chi = (t < L ? 2 * t + 1 : S - 1) >> 2;
    const double lse_t = is_prob ? 0.0 : u.lse[t];
    const size_t row = (size_t)t * (size_t)V;
    const double e_blank = align_emit(u.x, dtype, row + (size_t)blank, lse_t, is_prob, clip_lo);
    for (int c = clo + cx.tid; c <= chi; c += cx.nt) {
      const int s0 = 4 * c, k0 = 2 * c, k1 = 2 * c + 1;
      const int l0 = k0 < L ? u.lab[k0] : -1, l1 = k1 < L ? u.lab[k1] : -1;
      const int lm1 = k0 > 0 && k0 <= L ? u.lab[k0 - 1] : -1;
      const double pm1 = s0 - 1 >= prev_lo4 ? prev[s0 - 1] : NEG;
      const double p0 = prev[s0], p1 = prev[s0 + 1], p2 = prev[s0 + 2], p3 = prev[s0 + 3];
      // blank s0: stay / step
      double b0 = p0;
      unsigned q4 = 0;
      if (pm1 > b0) b0 = pm1, q4 = 1u;
      cur[s0] = b0 + e_blank;
      // label k0: stay / step / skip over the blank when the label before differs
      double b1 = NEG, b2 = NEG, b3 = NEG;
      if (l0 >= 0) {
        unsigned q = 0;
        b1 = p1;
        if (p0 > b1) b1 = p0, q = 1u;
        if (lm1 >= 0 && lm1 != l0 && pm1 > b1) b1 = pm1, q = 2u;
        q4 |= q << 2;
        b1 += align_emit(u.x, dtype, row + (size_t)l0, lse_t, is_prob, clip_lo);
      }
      if (s0 + 2 < S) {
        unsigned q = 0;
        b2 = p2;
        if (p1 > b2) b2 = p1, q = 1u;
        q4 |= q << 4;
        b2 += e_blank;
      }
      if (l1 >= 0) {
        unsigned q = 0;
        b3 = p3;
        if (p2 > b3) b3 = p2, q = 1u;
        if (l1 != l0 && p1 > b3) b3 = p1, q = 2u;
        q4 |= q << 6;
        b3 += align_emit(u.x, dtype, row + (size_t)l1, lse_t, is_prob, clip_lo);
      }
      cur[s0 + 1] = b1;
      cur[s0 + 2] = b2;
      cur[s0 + 3] = b3;
      if (BP) bp[(size_t)(t - f - 1) * (size_t)nch + (size_t)c] = (uint8_t)q4;
    }
    prev_lo4 = 4 * clo;
    cx.sync();  // the one barrier of a frame: the columns swap roles
  }
}

// cx: tid, nt, sync(). A thread loops over its groups of four states as in ctc_viterbi_utt; a workgroup reads from device
// memory only what it wrote itself, behind a barrier.
template <class Ctx>
CTC_HD void ctc_viterbi_long_utt(Ctx& cx, const AlignLongUtt& u, int V, int dtype, int blank, int fold, double clip_lo) {
  const int T = u.T, L = u.L, K = u.K;
  if (T <= 0) return;
  const int S = 2 * L + 1, nch = align_chunks(L), nseg = align_long_segments(T, K);
  const double NEG = align_neg_inf();
  const bool is_prob = u.is_prob != 0;
  double* c0 = u.col;
  double* c1 = u.col + 4 * nch;
  for (int i = cx.tid; i < 8 * nch; i += cx.nt) u.col[i] = NEG;
  cx.sync();
  if (cx.tid == 0) {
    const double lse0 = is_prob ? 0.0 : u.lse[0];
    c0[0] = align_emit(u.x, dtype, (size_t)blank, lse0, is_prob, clip_lo);
    if (L > 0) c0[1] = align_emit(u.x, dtype, (size_t)u.lab[0], lse0, is_prob, clip_lo);
  }
  cx.sync();
  // the pass over all frames. What lies above a frame's window in either column still holds the -inf written above: a
  // checkpoint is the whole column, those cells included.
  for (int j = 0; j < nseg; ++j) {
    const int f = j * K, e = align_long_segment_end(T, K, f);
    if (nseg == 1) {
      viterbi_long_frames<true>(cx, u, V, dtype, blank, clip_lo, f, e, u.bp);
    } else {
      const double* at = (f & 1) ? c1 : c0;  // (complete behind frame f's barrier; next written by frame f + 2, behind frame f + 1's)
      double* keep = u.ckpt + (size_t)j * (size_t)(4 * nch);
      for (int i = cx.tid; i < 4 * nch; i += cx.nt) keep[i] = at[i];
      viterbi_long_frames<false>(cx, u, V, dtype, blank, clip_lo, f, e, nullptr);
    }
  }
  // the end state and the score, by the thread that traces back: the last label is preferred over the trailing blank, and
  // the score is the last column's value -- nothing is summed a second time
  int s = 0, open = -1;
  if (cx.tid == 0) {
    const double* fin = ((T - 1) & 1) ? c1 : c0;
    s = (L > 0 && fin[S - 2] >= fin[S - 1]) ? S - 2 : S - 1;
    *u.score = fin[s];
  }
  const auto slot = [&](int) { return blank; };
  if (nseg == 1) {
    if (cx.tid == 0) viterbi_backtrace_span(s, open, T - 1, 1, 1, nch, u.bp, u.lab, u.path, u.tok_start, u.tok_end, slot);
  } else {
    for (int j = nseg - 1; j >= 0; --j) {
      const int f = j * K, e = align_long_segment_end(T, K, f);
      double* at = (f & 1) ? c1 : c0;
      double* other = (f & 1) ? c0 : c1;
      const double* keep = u.ckpt + (size_t)j * (size_t)(4 * nch);
      cx.sync();  // (thread 0 has read the last column)
      // The other column would hold what a later frame left there, above frame f's window too, where frame f + 2 expects
      // -inf: all of it is reset. Below the window nothing is read, inside it frame f + 1 writes first.
      for (int i = cx.tid; i < 4 * nch; i += cx.nt) at[i] = keep[i], other[i] = NEG;
      cx.sync();  // (and thread 0 is through with the table of the segment above)
      viterbi_long_frames<true>(cx, u, V, dtype, blank, clip_lo, f, e, u.bp);
      // s and open go on into the segment below: a label's span may cross the boundary
      if (cx.tid == 0) viterbi_backtrace_span(s, open, e, f + 1, f + 1, nch, u.bp, u.lab, u.path, u.tok_start, u.tok_end, slot);
    }
  }
  if (cx.tid == 0) viterbi_backtrace_span(s, open, 0, 0, 0, nch, u.bp, u.lab, u.path, u.tok_start, u.tok_end, slot);  // frame 0: no step
  if (!fold) return;
  cx.sync();  // (the spans thread 0 wrote are read by every thread)
  fold_token_logp(cx, u.x, dtype, u.lse, u.lab, u.tok_start, u.tok_end, u.tok_logp, T, L, V, is_prob, fold, clip_lo);
}

// ---- ctc_forward / ctc_forward_wave ----------------------------------------------------------------------------------------
// The likelihood of a label sequence: over the states and the reachable-state window of ctc_viterbi,
//   a_t[s] = lse3(a_{t-1}[s], a_{t-1}[s-1], skip ? a_{t-1}[s-2] : -inf) + emit(t, s),   result = lse2(a_{T-1}[S-1], a_{T-1}[S-2]).
// One hypothesis of a launch. The host validates every field before a launch as for AlignUtt (T >= L + repeats >= 1).
struct ForwardHyp {
  const void* x;       // [T, V] logits or probabilities of the hypothesis' utterance, of the launch's dtype
  const double* lse;   // [T] log-sum-exp of each row (not read when is_prob)
  const int32_t* lab;  // [L] the labels scored
  double* logp;        // [1] out
  int32_t T, L, is_prob, pad;
};

// What the forward bodies leave behind per frame when they run for ctc_prefix_extend (ENDS; "ctc_prefix_extend" below):
//   bc[t]     = a_{t-1}[S-1]   the target is complete and the frame before was a blank   (t = 0: -inf)
//   bc[T + t] = a_{t-1}[S-2]   the target is complete and the frame before was its last label (t = 0: 0 for the empty target)
// and scale[0], the largest of these 2T values: -inf when the target cannot be complete before the last frame.
struct PrefixEnds {
  double* bc;     // [2 T] out
  double* scale;  // [1] out
};

constexpr int32_t FORWARD_MAX_GROUPS = (2 * ALIGN_MAX_LABELS + 1 + 3) / 4;  // align_chunks(ALIGN_MAX_LABELS)
constexpr int32_t FORWARD_WAVE_MAX_LABELS = 127;  // ctc_forward_wave: 2L + 1 <= 256 states, four to each of a wave's 64 lanes

// log(exp(stay) + exp(step) + exp(skip)): the maximum first, then the sum in that fixed order; -inf when all three are.
// No multiplication: contraction has nothing to fuse, and every caller gets the same bits from the same operands. An
// operand of -inf adds exactly 0, with or without its exp (a blank's skip is the constant -inf: its exp compiles away).
CTC_HD double align_lse3(double stay, double step, double skip) {
  const double NEG = align_neg_inf();
  double m = stay > step ? stay : step;
  m = skip > m ? skip : m;
  if (!(m > NEG)) return NEG;
  double s = stay > NEG ? exp(stay - m) : 0.0;
  s += step > NEG ? exp(step - m) : 0.0;
  s += skip > NEG ? exp(skip - m) : 0.0;
  return m + log(s);
}
CTC_HD double align_lse2(double a, double b) { return align_lse3(a, b, align_neg_inf()); }

// What a group of four states (blank, label 2c, blank, label 2c + 1) keeps for the whole recursion: its labels (-1: the
// target ends before them) and whether each may be entered over the blank before it.
struct ForwardGroup {
  int32_t l0, l1;
  bool skip0, skip1, blank2;  // label 2c differs from label 2c - 1; label 2c + 1 from label 2c; the state 4c + 2 exists
};
CTC_HD ForwardGroup forward_group(const int32_t* lab, int L, int c) {
  const int k0 = 2 * c, k1 = 2 * c + 1;
  ForwardGroup g;
  g.l0 = k0 < L ? lab[k0] : -1;
  g.l1 = k1 < L ? lab[k1] : -1;
  const int lm1 = k0 > 0 && k0 <= L ? lab[k0 - 1] : -1;
  g.skip0 = g.l0 >= 0 && lm1 >= 0 && lm1 != g.l0;
  g.skip1 = g.l1 >= 0 && g.l1 != g.l0;
  g.blank2 = 4 * c + 2 < 2 * L + 1;
  return g;
}
// One frame of one group, in place: p[0..3] the group's states at the frame before, pm1 the last state of the group below
// (it serves the blank's step and the first label's skip), e_* the frame's emissions.
CTC_HD void forward_step(const ForwardGroup& g, double pm1, double e_blank, double e0, double e1, double* p) {
  const double NEG = align_neg_inf();
  const double p0 = p[0], p1 = p[1], p2 = p[2], p3 = p[3];
  p[0] = align_lse2(p0, pm1) + e_blank;
  p[1] = g.l0 >= 0 ? align_lse3(p1, p0, g.skip0 ? pm1 : NEG) + e0 : NEG;
  p[2] = g.blank2 ? align_lse2(p2, p1) + e_blank : NEG;
  p[3] = g.l1 >= 0 ? align_lse3(p3, p2, g.skip1 ? p1 : NEG) + e1 : NEG;
}
// The groups that hold a state reachable from the start and from the end at frame t: [lo, hi] (ctc_viterbi's window)
CTC_HD void forward_window(int t, int T, int S, int* clo, int* chi) {
  const int lo = S - 2 - 2 * (T - 1 - t), hi = 2 * t + 1;
  *clo = lo > 0 ? lo >> 2 : 0;
  *chi = (hi < S - 1 ? hi : S - 1) >> 2;
}

// An entry of a matrix of dtype code DT as it lies in memory, and its (exact) widening to double. The forward kernels ask for
// a frame's entries one frame ahead and keep them as loaded: a conversion at the load would make the load's latency wait there.
template <int DT> struct AlignRaw { typedef uint16_t type; };
template <> struct AlignRaw<0> { typedef float type; };
template <> struct AlignRaw<1> { typedef double type; };
template <int DT>
CTC_HD typename AlignRaw<DT>::type align_load_raw(const void* x, size_t i) { return ((const typename AlignRaw<DT>::type*)x)[i]; }
template <int DT>
CTC_HD double align_widen(typename AlignRaw<DT>::type r) {
  if (DT == 0 || DT == 1) return (double)r;
  return (double)(DT == 2 ? f16_bits_to_f32((uint16_t)r) : bf16_bits_to_f32((uint16_t)r));
}
// (host) f(std::integral_constant<int, DT>()) for a dtype code: how a launcher, or the simulator, picks an instantiation
template <class F>
void for_dtype(int dtype, F f) {
  if (dtype == 0) f(std::integral_constant<int, 0>());
  else if (dtype == 1) f(std::integral_constant<int, 1>());
  else if (dtype == 2) f(std::integral_constant<int, 2>());
  else f(std::integral_constant<int, 3>());
}

// ---- what the bodies with a group per thread (or lane) share -----------------------------------------------------------------
// Like ctc_forward and ctc_posteriors, ctc_find and ctc_viterbi_gaps give thread tid of cx (tid, nt, sync(); Ctx::GROUPS * nt >= the
// target's groups) the groups tid, tid + nt, ... for the whole recursion: their labels and skip flags are read once, their
// states stay in registers, and only a group's last state goes through LDS to the thread that owns the group above, one
// barrier per frame. ctc_forward_wave and ctc_find_wave give lane c group c and pass that state by a shuffle.

// Where a thread's entries come from, fixed for the recursion
template <int G>
struct EntrySource {
  const void* x;        // [T, V] the utterance's matrix
  const double* lse_v;  // [T] the rows' log-sum-exps (any valid address for probabilities: never used)
  const double* max_v;  // [T] the rows' maxima (ctc_viterbi_gaps; else null)
  int V, blank;
  bool is_prob;
  double clip_lo;
  int i0[G], i1[G];     // the columns each group's two labels read
};

// Group c of a target with nch groups: the ForwardGroup, or the empty group past the last one, and the columns its two
// labels read -- the blank's where the target ends before them, so that a load there is valid whatever the group
CTC_HD ForwardGroup group_setup(const int32_t* lab, int L, int nch, int c, int blank, int* i0, int* i1) {
  const ForwardGroup g = c < nch ? forward_group(lab, L, c) : ForwardGroup{-1, -1, false, false, false};
  *i0 = g.l0 >= 0 ? g.l0 : blank;
  *i1 = g.l1 >= 0 ? g.l1 : blank;
  return g;
}

// A thread's opening: its groups, and the source of its entries
template <class Ctx>
CTC_HD void thread_setup(const Ctx& cx, const void* x, const double* lse, const double* rmax, const int32_t* lab, int L, int nch, int V,
                         int blank, bool is_prob, double clip_lo, ForwardGroup* g, EntrySource<Ctx::GROUPS>& src) {
  CTC_UNROLL
  for (int k = 0; k < Ctx::GROUPS; ++k) g[k] = group_setup(lab, L, nch, cx.tid + k * cx.nt, blank, &src.i0[k], &src.i1[k]);
  // (always 0, but per thread as far as the compiler knows: a row's log-sum-exp -- and maximum -- then comes by a vector load
  // like the entries. Loaded at a workgroup-uniform address it would be a scalar load, which shares its counter with the LDS
  // reads: the wait for the neighbour's state would wait for the next frame's value as well.)
  const int per_thread_zero = g[0].l0 == -2 ? 1 : 0;
  src.x = x;
  src.lse_v = lse + per_thread_zero;
  src.max_v = rmax ? rmax + per_thread_zero : nullptr;
  src.V = V, src.blank = blank, src.is_prob = is_prob, src.clip_lo = clip_lo;
}

// A thread's entries of one frame, kept as loaded (AlignRaw). Nothing a recursion computes decides the entries of the frame
// after: a body asks for them -- request(): loads alone, without a branch, at indices that are always valid -- into a second
// instance after the neighbour's state is in hand and before the frame's arithmetic and barrier, and hands them over by
// assignment at the end of the frame.
template <int DT, int G, bool MAX = false>
struct FrameEntries {
  typedef typename AlignRaw<DT>::type Raw;
  Raw vb, v0[G], v1[G];  // the blank's entry, and those of each group's two labels
  double lse_t, max_t;   // the row's log-sum-exp and (MAX) maximum
  CTC_HD void request(const EntrySource<G>& s, int tn) {
    const size_t row = (size_t)tn * (size_t)s.V;
    vb = align_load_raw<DT>(s.x, row + (size_t)s.blank);
    lse_t = s.lse_v[tn];
    max_t = MAX ? s.max_v[tn] : 0.0;
    CTC_UNROLL
    for (int k = 0; k < G; ++k) {
      v0[k] = align_load_raw<DT>(s.x, row + (size_t)s.i0[k]);
      v1[k] = align_load_raw<DT>(s.x, row + (size_t)s.i1[k]);
    }
  }
  CTC_HD double emit(const EntrySource<G>& s, double v) const { return align_emit_of_value(v, s.is_prob ? 0.0 : lse_t, s.is_prob, s.clip_lo); }
  CTC_HD double emit_blank(const EntrySource<G>& s) const { return emit(s, align_widen<DT>(vb)); }
  CTC_HD double emit0(const EntrySource<G>& s, int k) const { return emit(s, align_widen<DT>(v0[k])); }
  CTC_HD double emit1(const EntrySource<G>& s, int k) const { return emit(s, align_widen<DT>(v1[k])); }
  CTC_HD double emit_max(const EntrySource<G>& s) const { return emit(s, max_t); }
};

// ctc_forward: the threads of cx (tid, nt, sync(); Ctx::GROUPS * nt >= align_chunks(L)) share one hypothesis of a matrix of
// dtype DT. Thread tid owns the groups tid, tid + nt, ... for the whole recursion: their labels and skip flags are read once,
// their states stay in registers, and only a group's last state goes through `col` (2 * align_chunks(L) doubles, the columns
// of two successive frames) to the thread that owns the group above: one barrier per frame. Nothing the recursion computes
// decides the entries of frame t + 1: they are requested -- without a branch, at indices that are always valid, and kept as
// loaded -- after the neighbour's state is in hand and before frame t's arithmetic and barrier.
// ENDS: the thread that owns the last group also stores, ahead of every frame's step, the two states a complete target ends
// in (PrefixEnds) -- two stores and two compares a frame, no arithmetic of the recursion changes.
template <int DT, bool ENDS = false, class Ctx>
CTC_HD void ctc_forward_hyp(Ctx& cx, const ForwardHyp& hyp, int V, int blank, double clip_lo, double* col, const PrefixEnds* ends = nullptr) {
  typedef typename AlignRaw<DT>::type Raw;
  constexpr int G = Ctx::GROUPS;
  const void* const x = hyp.x;  // (the record, once: the loop below reads none of it again)
  const double* const lse = hyp.lse;
  const int32_t* const lab = hyp.lab;
  double* const out = hyp.logp;
  const int T = hyp.T, L = hyp.L;
  const bool is_prob = hyp.is_prob != 0;
  if (T <= 0) return;
  const int S = 2 * L + 1, nch = align_chunks(L);
  const double NEG = align_neg_inf();
  ForwardGroup g[G];
  int i0[G], i1[G];  // the columns a group's two labels read (the blank's where the target ends before them)
  double p[G][4];    // states
  Raw v0[G], v1[G];  // the entries of the frame in hand at those columns, as loaded
  CTC_UNROLL
  for (int k = 0; k < G; ++k) {
    const int c = cx.tid + k * cx.nt;
    p[k][0] = p[k][1] = p[k][2] = p[k][3] = NEG;
    if (c < nch) g[k] = forward_group(lab, L, c);
    else g[k] = ForwardGroup{-1, -1, false, false, false};
    i0[k] = g[k].l0 >= 0 ? g[k].l0 : blank;
    i1[k] = g[k].l1 >= 0 ? g[k].l1 : blank;
  }
  // (always 0, but per thread as far as the compiler knows: a row's log-sum-exp then comes by a vector load like the entries.
  // Loaded at a workgroup-uniform address it would be a scalar load, which shares its counter with the LDS reads: the wait for
  // the neighbour's state would wait for the next frame's value as well.)
  const int per_thread_zero = g[0].l0 == -2 ? 1 : 0;
  const double* const lse_v = lse + per_thread_zero;
  for (int i = cx.tid; i < 2 * nch; i += cx.nt) col[i] = NEG;
  if (cx.tid == 0) {
    const double lse0 = is_prob ? 0.0 : lse[0];
    p[0][0] = align_emit(x, DT, (size_t)blank, lse0, is_prob, clip_lo);
    if (L > 0) p[0][1] = align_emit(x, DT, (size_t)lab[0], lse0, is_prob, clip_lo);
  }
  double ends_m = L == 0 ? 0.0 : NEG;  // (ENDS) the largest end state stored so far
  if constexpr (ENDS) {
    if (cx.tid == 0) ends->bc[0] = NEG, ends->bc[T] = ends_m;
  }
  cx.sync();
  // frame 1's entries (a single frame: frame 0's again, never used)
  int clo = 0, chi = -1, clo_prev = 0;
  if (T > 1) forward_window(1, T, S, &clo, &chi);
  const size_t row1 = T > 1 ? (size_t)V : 0;
  Raw vb = align_load_raw<DT>(x, row1 + (size_t)blank);
  double lse_t = lse_v[T > 1 ? 1 : 0];
  CTC_UNROLL
  for (int k = 0; k < G; ++k) {
    v0[k] = align_load_raw<DT>(x, row1 + (size_t)i0[k]);
    v1[k] = align_load_raw<DT>(x, row1 + (size_t)i1[k]);
  }
  for (int t = 1; t < T; ++t) {
    const double* prev = col + ((t - 1) & 1) * nch;
    double* cur = col + (t & 1) * nch;
    // the neighbours' states first: what lies below the window of the frame before is unreachable from the end and reads
    // as -inf, as in ctc_viterbi
    double pm1[G];
    CTC_UNROLL
    for (int k = 0; k < G; ++k) {
      const int c = cx.tid + k * cx.nt;
      pm1[k] = c >= clo && c <= chi && c > 0 && c - 1 >= clo_prev ? prev[c - 1] : NEG;
    }
    if constexpr (ENDS) {  // a_{t-1}[S-1] and a_{t-1}[S-2], read as the result below reads them (the window never cuts them off)
      const int ce = (S - 1) >> 2, je = (S - 1) & 3;
      CTC_UNROLL
      for (int k = 0; k < G; ++k) {
        if (cx.tid + k * cx.nt != ce) continue;
        const double last = je == 2 ? p[k][2] : p[k][0];
        const double before = je == 2 ? p[k][1] : (ce > 0 ? prev[ce - 1] : NEG);
        ends->bc[t] = last;
        ends->bc[T + t] = before;
        ends_m = last > ends_m ? last : ends_m;
        ends_m = before > ends_m ? before : ends_m;
      }
    }
    // then ask for frame t + 1 (after the last frame: the last frame again)
    const int tn = t + 1 < T ? t + 1 : t;
    int nlo = 0, nhi = -1;
    if (t + 1 < T) forward_window(tn, T, S, &nlo, &nhi);
    const size_t row = (size_t)tn * (size_t)V;
    const Raw nvb = align_load_raw<DT>(x, row + (size_t)blank);
    const double nlse = lse_v[tn];
    Raw n0[G], n1[G];
    CTC_UNROLL
    for (int k = 0; k < G; ++k) {
      n0[k] = align_load_raw<DT>(x, row + (size_t)i0[k]);
      n1[k] = align_load_raw<DT>(x, row + (size_t)i1[k]);
    }
    const double lse_use = is_prob ? 0.0 : lse_t;
    const double e_blank = align_emit_of_value(align_widen<DT>(vb), lse_use, is_prob, clip_lo);
    CTC_UNROLL
    for (int k = 0; k < G; ++k) {
      const int c = cx.tid + k * cx.nt;
      if (c < clo || c > chi) continue;
      const double e0 = align_emit_of_value(align_widen<DT>(v0[k]), lse_use, is_prob, clip_lo);
      const double e1 = align_emit_of_value(align_widen<DT>(v1[k]), lse_use, is_prob, clip_lo);
      forward_step(g[k], pm1[k], e_blank, e0, e1, p[k]);
      cur[c] = p[k][3];
    }
    clo_prev = clo;
    clo = nlo, chi = nhi, vb = nvb, lse_t = nlse;
    CTC_UNROLL
    for (int k = 0; k < G; ++k) v0[k] = n0[k], v1[k] = n1[k];
    cx.sync();  // the one barrier of a frame: the columns swap roles
  }
  // the last blank and the last label: state S - 1 = 2L is entry 0 or 2 of its group, S - 2 the entry before it
  const int cf = (S - 1) >> 2, jf = (S - 1) & 3;
  const double* fin = col + ((T - 1) & 1) * nch;
  CTC_UNROLL
  for (int k = 0; k < G; ++k) {
    if (cx.tid + k * cx.nt != cf) continue;
    const double last = jf == 2 ? p[k][2] : p[k][0];
    const double before = jf == 2 ? p[k][1] : (cf > 0 ? fin[cf - 1] : NEG);
    *out = align_lse2(last, before);
    if constexpr (ENDS) *ends->scale = ends_m;
  }
}

// ctc_forward_wave: one wavefront per hypothesis of at most FORWARD_WAVE_MAX_LABELS labels. Lane c owns group c; the last
// state of the group below comes from lane c - 1 by cx.up() (one fp64 shuffle per frame): no LDS, no barrier. The same
// groups, steps and prefetch as ctc_forward_hyp, so the same bits. cx: lane, up(v) = v of the lane below (any value in lane 0).
template <int DT, bool ENDS = false, class Ctx>
CTC_HD void ctc_forward_wave_hyp(Ctx& cx, const ForwardHyp& hyp, int V, int blank, double clip_lo, const PrefixEnds* ends = nullptr) {
  typedef typename AlignRaw<DT>::type Raw;
  const void* const x = hyp.x;
  const double* const lse = hyp.lse;
  const int32_t* const lab = hyp.lab;
  double* const out = hyp.logp;
  const int T = hyp.T, L = hyp.L, c = cx.lane;
  const bool is_prob = hyp.is_prob != 0;
  if (T <= 0) return;
  const int S = 2 * L + 1, nch = align_chunks(L);
  const double NEG = align_neg_inf();
  const ForwardGroup g = c < nch ? forward_group(lab, L, c) : ForwardGroup{-1, -1, false, false, false};
  const int i0 = g.l0 >= 0 ? g.l0 : blank, i1 = g.l1 >= 0 ? g.l1 : blank;
  double p[4] = {NEG, NEG, NEG, NEG};
  if (c == 0) {
    const double lse0 = is_prob ? 0.0 : lse[0];
    p[0] = align_emit(x, DT, (size_t)blank, lse0, is_prob, clip_lo);
    if (L > 0) p[1] = align_emit(x, DT, (size_t)lab[0], lse0, is_prob, clip_lo);
  }
  double ends_m = L == 0 ? 0.0 : NEG;  // (ENDS) the largest end state stored so far
  if constexpr (ENDS) {
    if (c == 0) ends->bc[0] = NEG, ends->bc[T] = ends_m;
  }
  int clo = 0, chi = -1, clo_prev = 0;
  if (T > 1) forward_window(1, T, S, &clo, &chi);
  const size_t row1 = T > 1 ? (size_t)V : 0;
  Raw vb = align_load_raw<DT>(x, row1 + (size_t)blank);
  Raw v0 = align_load_raw<DT>(x, row1 + (size_t)i0), v1 = align_load_raw<DT>(x, row1 + (size_t)i1);
  double lse_t = lse[T > 1 ? 1 : 0];
  for (int t = 1; t < T; ++t) {
    const double below = cx.up(p[3]);  // (every lane takes part, whatever its window says)
    if constexpr (ENDS) {  // a_{t-1}[S-1] and a_{t-1}[S-2], read as the result below reads them
      const int ce = (S - 1) >> 2, je = (S - 1) & 3;
      if (c == ce) {
        const double last = je == 2 ? p[2] : p[0];
        const double before = je == 2 ? p[1] : (ce > 0 ? below : NEG);
        ends->bc[t] = last;
        ends->bc[T + t] = before;
        ends_m = last > ends_m ? last : ends_m;
        ends_m = before > ends_m ? before : ends_m;
      }
    }
    const int tn = t + 1 < T ? t + 1 : t;
    int nlo = 0, nhi = -1;
    if (t + 1 < T) forward_window(tn, T, S, &nlo, &nhi);
    const size_t row = (size_t)tn * (size_t)V;
    const Raw nvb = align_load_raw<DT>(x, row + (size_t)blank);
    const Raw n0 = align_load_raw<DT>(x, row + (size_t)i0), n1 = align_load_raw<DT>(x, row + (size_t)i1);
    const double nlse = lse[tn];
    if (c >= clo && c <= chi) {
      const double pm1 = c > 0 && c - 1 >= clo_prev ? below : NEG;
      const double lse_use = is_prob ? 0.0 : lse_t;
      const double e_blank = align_emit_of_value(align_widen<DT>(vb), lse_use, is_prob, clip_lo);
      const double e0 = align_emit_of_value(align_widen<DT>(v0), lse_use, is_prob, clip_lo);
      const double e1 = align_emit_of_value(align_widen<DT>(v1), lse_use, is_prob, clip_lo);
      forward_step(g, pm1, e_blank, e0, e1, p);
    }
    clo_prev = clo;
    clo = nlo, chi = nhi, vb = nvb, lse_t = nlse, v0 = n0, v1 = n1;
  }
  const int cf = (S - 1) >> 2, jf = (S - 1) & 3;
  const double below = cx.up(p[3]);
  if (c == cf) {
    const double last = jf == 2 ? p[2] : p[0];
    const double before = jf == 2 ? p[1] : (cf > 0 ? below : NEG);
    *out = align_lse2(last, before);
    if constexpr (ENDS) *ends->scale = ends_m;
  }
}

// ---- ctc_posteriors ----------------------------------------------------------------------------------------------------------
// The frame posteriors of a label sequence ("Frame posteriors"): the CTC forward-backward over the states and the
// window of ctc_forward,
//   gamma[t, s] = exp(a_t[s] + b_t[s] - logp),
//   a: ctc_forward's recursion (it includes frame t's emission), logp: ctc_forward's result, bit for bit;
//   b_{T-1}[S-1] = b_{T-1}[S-2] = 0,
//   b_t[s] = lse3(b_{t+1}[s] + e(t+1, s), b_{t+1}[s+1] + e(t+1, s+1), skip(s+2) ? b_{t+1}[s+2] + e(t+1, s+2) : -inf)
// (b excludes frame t's emission), and exactly 0.0 for a state outside the window S - 2 - 2 (T - 1 - t) <= s <= 2 t + 1.
// One utterance of a launch. The host validates every field before a launch as for AlignUtt (T >= L + repeats >= 1).
struct PostUtt {
  const void* x;       // [T, V] logits or probabilities, of the launch's dtype
  const double* lse;   // [T] log-sum-exp of each row (not read when is_prob)
  const int32_t* lab;  // [L] target labels
  double* table;       // [T][4 * align_chunks(L)], 16-byte aligned: a of the forward pass, overwritten by gamma when dense
  double* logp;        // [2] out: the forward score, and the same quantity read off frame 0 of the backward pass
  double* occ;         // [L] out: sum over t of gamma[t, 2k + 1]
  double* centre;      // [L] out: sum over t of t * gamma[t, 2k + 1], over occ[k]
  int32_t T, L, is_prob, pad;
};

// a group's four states as they lie in the table: one 32-byte slot, moved as two 16-byte halves that stay in registers
typedef double PostPair __attribute__((vector_size(16)));
CTC_HD void post_store(double* slot, double v0, double v1, double v2, double v3) {
  ((PostPair*)slot)[0] = PostPair{v0, v1};
  ((PostPair*)slot)[1] = PostPair{v2, v3};
}
CTC_HD size_t post_slot(int t, int nch, int c) { return ((size_t)t * (size_t)nch + (size_t)c) * 4; }

// One frame of one group of the backward pass, in place. In: q[0..3] = b + e of the group's states at the frame after, up0 /
// up1 the same of the first blank and the first label of the group above (-inf where there is none), skip_up: that label
// differs from this group's second. Out: q[0..3] = b of this frame. A state the target does not have stays -inf.
CTC_HD void backward_step(const ForwardGroup& g, bool skip_up, double up0, double up1, double* q) {
  const double NEG = align_neg_inf();
  const double q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
  q[0] = align_lse3(q0, q1, NEG);
  q[1] = g.l0 >= 0 ? align_lse3(q1, q2, g.skip1 ? q3 : NEG) : NEG;
  q[2] = g.blank2 ? align_lse3(q2, q3, NEG) : NEG;
  q[3] = g.l1 >= 0 ? align_lse3(q3, up0, skip_up ? up1 : NEG) : NEG;
}

// ctc_posteriors: the threads of cx (tid, nt, sync(); Ctx::GROUPS * nt >= align_chunks(L)) share one utterance of a matrix of
// dtype DT; thread tid owns the groups tid, tid + nt, ... for the whole call. `col`: 4 * align_chunks(L) + 2 doubles.
// Forward: ctc_forward_hyp's loop, operand for operand, which also stores the four a of every in-window group of every frame
// into the table. Backward, t = T - 1 .. 0: a group's b + e stay in registers; the first two go through two columns of `col`
// that swap roles every frame to the thread that owns the group below (one barrier per frame). The a row and the entries of
// frame t - 1 depend on nothing the recursion computes: they are requested one frame ahead, at slots that are always inside
// the window, and kept as loaded. gamma overwrites a in its own slot, by the thread that wrote it; with `dense` every
// out-of-window state of every frame (the padding of the last group included) is written as 0.0 -- the table comes from a
// workspace that holds stale data, so the forward pass writes and the backward pass reads in-window slots only. A thread sums
// gamma and t * gamma of its two labels in registers, in the order of the frames, and writes them once after frame 0.
template <int DT, class Ctx>
CTC_HD void ctc_posteriors_utt(Ctx& cx, const PostUtt& utt, int V, int blank, double clip_lo, int dense, double* col) {
  typedef typename AlignRaw<DT>::type Raw;
  constexpr int G = Ctx::GROUPS;
  const void* const x = utt.x;  // (the record, once: the loops below read none of it again)
  const double* const lse = utt.lse;
  const int32_t* const lab = utt.lab;
  double* const table = utt.table;
  double* const out = utt.logp;
  const int T = utt.T, L = utt.L;
  const bool is_prob = utt.is_prob != 0;
  if (T <= 0) return;
  const int S = 2 * L + 1, nch = align_chunks(L);
  const double NEG = align_neg_inf();
  ForwardGroup g[G];
  bool skip_up[G];   // the first label of the group above differs from this group's second
  int i0[G], i1[G];  // the columns a group's two labels read (the blank's where the target ends before them)
  double p[G][4];    // the forward pass' states
  Raw v0[G], v1[G];  // the entries of the frame in hand at those columns, as loaded
  CTC_UNROLL
  for (int k = 0; k < G; ++k) {
    const int c = cx.tid + k * cx.nt;
    p[k][0] = p[k][1] = p[k][2] = p[k][3] = NEG;
    if (c < nch) g[k] = forward_group(lab, L, c);
    else g[k] = ForwardGroup{-1, -1, false, false, false};
    skip_up[k] = g[k].l1 >= 0 && 2 * c + 2 < L && lab[2 * c + 2] != g[k].l1;
    i0[k] = g[k].l0 >= 0 ? g[k].l0 : blank;
    i1[k] = g[k].l1 >= 0 ? g[k].l1 : blank;
  }
  const int per_thread_zero = g[0].l0 == -2 ? 1 : 0;  // (ctc_forward_hyp: a row's log-sum-exp by a vector load)
  const double* const lse_v = lse + per_thread_zero;
  for (int i = cx.tid; i < 2 * nch; i += cx.nt) col[i] = NEG;
  if (cx.tid == 0) {
    const double lse0 = is_prob ? 0.0 : lse[0];
    p[0][0] = align_emit(x, DT, (size_t)blank, lse0, is_prob, clip_lo);
    if (L > 0) p[0][1] = align_emit(x, DT, (size_t)lab[0], lse0, is_prob, clip_lo);
    post_store(table + post_slot(0, nch, 0), p[0][0], p[0][1], p[0][2], p[0][3]);  // (frame 0's window: group 0)
  }
  cx.sync();
  int clo = 0, chi = -1, clo_prev = 0;
  if (T > 1) forward_window(1, T, S, &clo, &chi);
  const size_t row1 = T > 1 ? (size_t)V : 0;
  Raw vb = align_load_raw<DT>(x, row1 + (size_t)blank);
  double lse_t = lse_v[T > 1 ? 1 : 0];
  CTC_UNROLL
  for (int k = 0; k < G; ++k) {
    v0[k] = align_load_raw<DT>(x, row1 + (size_t)i0[k]);
    v1[k] = align_load_raw<DT>(x, row1 + (size_t)i1[k]);
  }
  for (int t = 1; t < T; ++t) {
    const double* prev = col + ((t - 1) & 1) * nch;
    double* cur = col + (t & 1) * nch;
    double pm1[G];
    CTC_UNROLL
    for (int k = 0; k < G; ++k) {
      const int c = cx.tid + k * cx.nt;
      pm1[k] = c >= clo && c <= chi && c > 0 && c - 1 >= clo_prev ? prev[c - 1] : NEG;
    }
    const int tn = t + 1 < T ? t + 1 : t;
    int nlo = 0, nhi = -1;
    if (t + 1 < T) forward_window(tn, T, S, &nlo, &nhi);
    const size_t row = (size_t)tn * (size_t)V;
    const Raw nvb = align_load_raw<DT>(x, row + (size_t)blank);
    const double nlse = lse_v[tn];
    Raw n0[G], n1[G];
    CTC_UNROLL
    for (int k = 0; k < G; ++k) {
      n0[k] = align_load_raw<DT>(x, row + (size_t)i0[k]);
      n1[k] = align_load_raw<DT>(x, row + (size_t)i1[k]);
    }
    const double lse_use = is_prob ? 0.0 : lse_t;
    const double e_blank = align_emit_of_value(align_widen<DT>(vb), lse_use, is_prob, clip_lo);
    CTC_UNROLL
    for (int k = 0; k < G; ++k) {
      const int c = cx.tid + k * cx.nt;
      if (c < clo || c > chi) continue;
      const double e0 = align_emit_of_value(align_widen<DT>(v0[k]), lse_use, is_prob, clip_lo);
      const double e1 = align_emit_of_value(align_widen<DT>(v1[k]), lse_use, is_prob, clip_lo);
      forward_step(g[k], pm1[k], e_blank, e0, e1, p[k]);
      cur[c] = p[k][3];
      post_store(table + post_slot(t, nch, c), p[k][0], p[k][1], p[k][2], p[k][3]);
    }
    clo_prev = clo;
    clo = nlo, chi = nhi, vb = nvb, lse_t = nlse;
    CTC_UNROLL
    for (int k = 0; k < G; ++k) v0[k] = n0[k], v1[k] = n1[k];
    cx.sync();  // the one barrier of a frame: the columns swap roles
  }
  // logp, formed as ctc_forward_hyp forms it, and handed to every thread
  const int cf = (S - 1) >> 2, jf = (S - 1) & 3;
  const double* fin = col + ((T - 1) & 1) * nch;
  double* const share = col + 4 * nch;
  CTC_UNROLL
  for (int k = 0; k < G; ++k) {
    if (cx.tid + k * cx.nt != cf) continue;
    const double last = jf == 2 ? p[k][2] : p[k][0];
    const double before = jf == 2 ? p[k][1] : (cf > 0 ? fin[cf - 1] : NEG);
    const double sum = align_lse2(last, before);
    out[0] = sum;
    share[0] = sum;
  }
  cx.sync();
  const double logp = share[0];

  // ---- backward ----
  double bq[G][4];  // the backward pass' states, with their frame's emissions: b + e
  double occ0[G], occ1[G], cen0[G], cen1[G];
  PostPair a01[G], a23[G];  // a of the frame in hand, as loaded
  CTC_UNROLL
  for (int k = 0; k < G; ++k) {
    bq[k][0] = bq[k][1] = bq[k][2] = bq[k][3] = NEG;
    occ0[k] = occ1[k] = cen0[k] = cen1[k] = 0.0;
  }
  // frame T - 1's entries and a (what a thread reads here it wrote itself)
  forward_window(T - 1, T, S, &clo, &chi);
  {
    const size_t row = (size_t)(T - 1) * (size_t)V;
    vb = align_load_raw<DT>(x, row + (size_t)blank);
    lse_t = lse_v[T - 1];
    CTC_UNROLL
    for (int k = 0; k < G; ++k) {
      const int c = cx.tid + k * cx.nt;
      const int cc = c < clo ? clo : (c > chi ? chi : c);
      v0[k] = align_load_raw<DT>(x, row + (size_t)i0[k]);
      v1[k] = align_load_raw<DT>(x, row + (size_t)i1[k]);
      a01[k] = ((const PostPair*)(table + post_slot(T - 1, nch, cc)))[0];
      a23[k] = ((const PostPair*)(table + post_slot(T - 1, nch, cc)))[1];
    }
  }
  int chi_next = -1;  // the last group of the window of the frame after
  for (int t = T - 1; t >= 0; --t) {
    const double* prev = col + ((t + 1) & 1) * 2 * nch;
    double* cur = col + (t & 1) * 2 * nch;
    // the group above first: beyond the window of the frame after there is nothing a state of this frame's window needs
    double up0[G], up1[G];
    CTC_UNROLL
    for (int k = 0; k < G; ++k) {
      const int c = cx.tid + k * cx.nt;
      const bool have = c >= clo && c <= chi && c + 1 <= chi_next;
      up0[k] = have ? prev[2 * (c + 1)] : NEG;
      up1[k] = have ? prev[2 * (c + 1) + 1] : NEG;
    }
    // then ask for frame t - 1 (before frame 0: frame 0 again)
    const int tn = t > 0 ? t - 1 : 0;
    int nlo, nhi;
    forward_window(tn, T, S, &nlo, &nhi);
    const size_t row = (size_t)tn * (size_t)V;
    const Raw nvb = align_load_raw<DT>(x, row + (size_t)blank);
    const double nlse = lse_v[tn];
    Raw n0[G], n1[G];
    PostPair na01[G], na23[G];
    CTC_UNROLL
    for (int k = 0; k < G; ++k) {
      const int c = cx.tid + k * cx.nt;
      const int cc = c < nlo ? nlo : (c > nhi ? nhi : c);
      n0[k] = align_load_raw<DT>(x, row + (size_t)i0[k]);
      n1[k] = align_load_raw<DT>(x, row + (size_t)i1[k]);
      na01[k] = ((const PostPair*)(table + post_slot(tn, nch, cc)))[0];
      na23[k] = ((const PostPair*)(table + post_slot(tn, nch, cc)))[1];
    }
    const double lse_use = is_prob ? 0.0 : lse_t;
    const double e_blank = align_emit_of_value(align_widen<DT>(vb), lse_use, is_prob, clip_lo);
    const int lo = S - 2 - 2 * (T - 1 - t), hi = 2 * t + 1 < S - 1 ? 2 * t + 1 : S - 1;
    const double ft = (double)t;
    CTC_UNROLL
    for (int k = 0; k < G; ++k) {
      const int c = cx.tid + k * cx.nt;
      if (c < clo || c > chi) {
        if (dense && c < nch) post_store(table + post_slot(t, nch, c), 0.0, 0.0, 0.0, 0.0);
        continue;
      }
      double* q = bq[k];
      const int s0 = 4 * c;
      if (t == T - 1) {
        q[0] = (s0 == S - 1 || s0 == S - 2) ? 0.0 : NEG;
        q[1] = (s0 + 1 == S - 1 || s0 + 1 == S - 2) ? 0.0 : NEG;
        q[2] = (s0 + 2 == S - 1 || s0 + 2 == S - 2) ? 0.0 : NEG;
        q[3] = (s0 + 3 == S - 1 || s0 + 3 == S - 2) ? 0.0 : NEG;
      } else {
        backward_step(g[k], skip_up[k], up0[k], up1[k], q);
      }
      const double gm0 = (s0 < lo || s0 > hi) ? 0.0 : exp(a01[k][0] + q[0] - logp);
      const double gm1 = (s0 + 1 < lo || s0 + 1 > hi) ? 0.0 : exp(a01[k][1] + q[1] - logp);
      const double gm2 = (s0 + 2 < lo || s0 + 2 > hi) ? 0.0 : exp(a23[k][0] + q[2] - logp);
      const double gm3 = (s0 + 3 < lo || s0 + 3 > hi) ? 0.0 : exp(a23[k][1] + q[3] - logp);
      if (dense) post_store(table + post_slot(t, nch, c), gm0, gm1, gm2, gm3);
      occ0[k] += gm1;
      cen0[k] += ft * gm1;
      occ1[k] += gm3;
      cen1[k] += ft * gm3;
      const double e0 = align_emit_of_value(align_widen<DT>(v0[k]), lse_use, is_prob, clip_lo);
      const double e1 = align_emit_of_value(align_widen<DT>(v1[k]), lse_use, is_prob, clip_lo);
      q[0] += e_blank;
      q[1] += e0;
      q[2] += e_blank;
      q[3] += e1;
      cur[2 * c] = q[0];
      cur[2 * c + 1] = q[1];
    }
    chi_next = chi;
    clo = nlo, chi = nhi, vb = nvb, lse_t = nlse;
    CTC_UNROLL
    for (int k = 0; k < G; ++k) v0[k] = n0[k], v1[k] = n1[k], a01[k] = na01[k], a23[k] = na23[k];
    cx.sync();  // the one barrier of a frame: the columns swap roles
  }
  CTC_UNROLL
  for (int k = 0; k < G; ++k) {
    const int c = cx.tid + k * cx.nt;
    if (c == 0) out[1] = align_lse2(bq[k][0], bq[k][1]);  // b_0 + e(0, .) of the two states a path may start in
    if (g[k].l0 >= 0) utt.occ[2 * c] = occ0[k], utt.centre[2 * c] = cen0[k] / occ0[k];
    if (g[k].l1 >= 0) utt.occ[2 * c + 1] = occ1[k], utt.centre[2 * c + 1] = cen1[k] / occ1[k];
  }
}

// ---- ctc_grad_rows -----------------------------------------------------------------------------------------------------------
// The gradient of ctc_forward's logp with respect to the utterance's own matrix ("Transcript gradient"), one row
// (t, utterance) at a time, from the gamma a dense ctc_posteriors launch left in the utterance's table. With G[t, k] the sum
// of gamma[t, s] over the states s whose label is k, and e the emission of align_emit_of_value:
//   logits:        u = (x - lse >= clip_lo), G' = u G, M = sum_k G'[t, k],  grad[t, v] = G'[t, v] - exp(x[t, v] - lse[t]) M
//   probabilities: grad[t, v] = 1e-15 <= p <= 1 ? G[t, v] / p : 0
// (the clip has derivative 0 where it holds: a NaN or -inf entry has u = 0). Nothing is scattered: the host lists, per
// utterance, the states of every label (occ_off[v] .. occ_off[v + 1] of occ_state, ascending), and the thread that owns entry
// v sums its list in that order. One utterance of a launch, validated by the host like PostUtt.
struct GradUtt {
  const void* x;             // [T, V] logits or probabilities, of the launch's dtype
  const double* lse;         // [T] log-sum-exp of each row (not read when is_prob)
  const double* table;       // [T][4 * align_chunks(L)] gamma, 0.0 outside the window (a dense ctc_posteriors launch wrote it)
  const int32_t* occ_off;    // [V + 1] label v is the target's labels occ_off[v] .. occ_off[v + 1] in occ_state (the blank: none)
  const int32_t* occ_state;  // [L] state indices 2 k + 1, ascending within a label
  void* grad;                // [T, V] out, of the launch's gradient type
  int64_t row_begin;         // the utterance's first row among the rows of the launch
  int32_t T, L, is_prob, pad;
};

// 1.0 where the emission is not held by its clip, else 0.0
CTC_HD double grad_unclipped(double v, double lse, bool is_prob, double clip_lo) {
  if (is_prob) return (v >= 1e-15 && v <= 1.0) ? 1.0 : 0.0;
  return (v - lse >= clip_lo) ? 1.0 : 0.0;
}
// G[t, v] of a label: its states inside the window [lo, hi], in ascending order (outside it gamma is 0.0: skipping adds the same)
CTC_HD double grad_label_sum(const double* gamma, const int32_t* occ_off, const int32_t* occ_state, int v, int lo, int hi) {
  double acc = 0.0;
  const int j1 = occ_off[v + 1];
  for (int j = occ_off[v]; j < j1; ++j) {
    const int s = occ_state[j];
    if (s >= lo && s <= hi) acc += gamma[s];
  }
  return acc;
}
// u G (logits) or G / p (probabilities) of entry v, whose value is xv. Only the blank and the target's labels have a G.
CTC_HD double grad_share(const GradUtt& u, const double* gamma, int v, int blank, double g_blank, double xv, double lse, double clip_lo,
                         int lo, int hi) {
  const bool is_prob = u.is_prob != 0;
  const double g = v == blank ? g_blank : grad_label_sum(gamma, u.occ_off, u.occ_state, v, lo, hi);
  if (grad_unclipped(xv, lse, is_prob, clip_lo) == 0.0) return 0.0;
  return is_prob ? g / xv : g;
}

// One row. cx: tid, nt (the threads that share the row), KEEP (entries a thread keeps in registers between the two passes),
// sum(v, slot): the sum of v over the nt threads in a fixed tree, the same bits in every thread. Thread tid owns the entries
// tid, tid + nt, ...: pass one loads each once, forms its share and adds it to the thread's part of M; pass two writes. What
// lies beyond KEEP * nt entries is formed again in pass two, with the same operands. The blank's G is the sum of the even
// states of the window: thread tid takes the states 2 (tid + i nt) in ascending i, and sum() folds the parts.
template <int DT, class GT, class Ctx>
CTC_HD void ctc_grad_row(Ctx& cx, const GradUtt& u, int t, int V, int blank, double clip_lo) {
  constexpr int K = Ctx::KEEP;
  const int T = u.T, S = 2 * u.L + 1, nch = align_chunks(u.L);
  const bool is_prob = u.is_prob != 0;
  const double* const gamma = u.table + post_slot(t, nch, 0);
  const int lo_raw = S - 2 - 2 * (T - 1 - t), lo = lo_raw > 0 ? lo_raw : 0, hi = 2 * t + 1 < S - 1 ? 2 * t + 1 : S - 1;
  double part = 0.0;
  for (int s = ((lo + 1) & ~1) + 2 * cx.tid; s <= hi; s += 2 * cx.nt) part += gamma[s];
  const double g_blank = cx.sum(part, 0);
  const double lse = is_prob ? 0.0 : u.lse[t];
  const size_t row = (size_t)t * (size_t)V;
  GT* const out = (GT*)u.grad + row;
  double xv[K], share[K];
  double m = 0.0;
  CTC_UNROLL
  for (int k = 0; k < K; ++k) {
    const int v = cx.tid + k * cx.nt;
    xv[k] = share[k] = 0.0;
    if (v >= V) continue;
    xv[k] = align_load(u.x, DT, row + (size_t)v);
    share[k] = grad_share(u, gamma, v, blank, g_blank, xv[k], lse, clip_lo, lo, hi);
    m += share[k];
  }
  for (int v = cx.tid + K * cx.nt; v < V; v += cx.nt)
    m += grad_share(u, gamma, v, blank, g_blank, align_load(u.x, DT, row + (size_t)v), lse, clip_lo, lo, hi);
  const double M = cx.sum(m, 1);
  CTC_UNROLL
  for (int k = 0; k < K; ++k) {
    const int v = cx.tid + k * cx.nt;
    if (v >= V) continue;
    out[v] = (GT)(is_prob ? share[k] : share[k] - exp(xv[k] - lse) * M);
  }
  for (int v = cx.tid + K * cx.nt; v < V; v += cx.nt) {
    const double x = align_load(u.x, DT, row + (size_t)v);
    const double sh = grad_share(u, gamma, v, blank, g_blank, x, lse, clip_lo, lo, hi);
    out[v] = (GT)(is_prob ? sh : sh - exp(x - lse) * M);
  }
}

// ---- ctc_find / ctc_find_wave -----------------------------------------------------------------------------------------------
// Where a phrase occurs in an utterance, and how well ("Phrase search"): the Viterbi recursion over the states of
// ctc_viterbi with a free start and a free end. Only the interior states 1 .. S - 2 exist -- an occurrence begins on a frame
// of the first label and ends on a frame of the last --, every one of them in every frame, and each carries the frame its
// path began on along with its score: d[s], st[s]. In frame t state s takes the best of stay (d[s]), step (d[s-1], s >= 2),
// skip (d[s-2], s >= 3, a label that differs from the label before it) and, for s = 1 alone, a fresh start (0.0, begun at
// t), equal scores preferring the earlier in that order, and adds emit(t, s); a state without a finite candidate is -inf.
// After frame t the trace holds end_logp[t] = d[S-2] and end_start[t] = st[S-2] (-inf / -1): the best occurrence whose last
// label sits on frame t. One phrase of a launch; the host validates every field before a launch (T >= L + repeats, L >= 1).
struct FindPhrase {
  const void* x;        // [T, V] logits or probabilities of the phrase's utterance, of the launch's dtype
  const double* lse;    // [T] log-sum-exp of each row (not read when is_prob)
  const int32_t* lab;   // [L] the labels searched for
  double* end_logp;     // [T] out: the trace's scores
  int32_t* end_start;   // [T] out: the trace's start frames
  double* hit_logp;     // [max_hits] out
  int32_t* hit_start;   // [max_hits] out
  int32_t* hit_end;     // [max_hits] out: one past the hit's last frame
  int32_t* n_hits;      // [1] out
  int32_t T, L, is_prob, pad;
};

constexpr int32_t FIND_MAX_HITS = 64;          // a wavefront keeps the windows taken so far one to a lane
constexpr int32_t FIND_WAVE_MAX_LABELS = 127;  // ctc_find_wave: 2L - 1 <= 253 interior states, four to each of a wave's 64 lanes
CTC_HD constexpr int32_t find_chunks(int32_t L) { return (L + 1) >> 1; }  // groups of four states that hold an interior state

// One frame of one group (blank, label 2c, blank, label 2c + 1: ForwardGroup), in place: d / st the group's scores and start
// frames at the frame before, dm1 / sm1 those of the last state of the group below. `first`: the group holds state 1, the only
// one a path may begin in; its state 0 does not exist. Nothing but compares and additions: the same operands give the same
// bits wherever this is inlined.
CTC_HD void find_step(const ForwardGroup& g, bool first, int t, double dm1, int32_t sm1, double e_blank, double e0, double e1,
                      double* d, int32_t* st) {
  const double NEG = align_neg_inf();
  const double d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3];
  const int32_t s0 = st[0], s1 = st[1], s2 = st[2], s3 = st[3];
  double b;
  int32_t bs;
  // blank 4c: stay / step
  b = d0, bs = s0;
  if (dm1 > b) b = dm1, bs = sm1;
  d[0] = !first && g.l0 >= 0 ? b + e_blank : NEG;
  st[0] = bs;
  // label 2c: stay / step / skip / a fresh start
  b = d1, bs = s1;
  if (d0 > b) b = d0, bs = s0;
  if (g.skip0 && dm1 > b) b = dm1, bs = sm1;
  if (first && 0.0 > b) b = 0.0, bs = t;
  d[1] = g.l0 >= 0 ? b + e0 : NEG;
  st[1] = bs;
  // blank 4c + 2 (interior when label 2c + 1 exists): stay / step
  b = d2, bs = s2;
  if (d1 > b) b = d1, bs = s1;
  d[2] = g.l1 >= 0 ? b + e_blank : NEG;
  st[2] = bs;
  // label 2c + 1: stay / step / skip
  b = d3, bs = s3;
  if (d2 > b) b = d2, bs = s2;
  if (g.skip1 && d1 > b) b = d1, bs = s1;
  d[3] = g.l1 >= 0 ? b + e1 : NEG;
  st[3] = bs;
}

// The selection, by one wavefront over the trace it wrote itself: until max_hits are taken or no end frame qualifies, the
// end frame t with the largest finite end_logp[t] >= min_logp whose window [end_start[t], t] shares no frame with a window
// taken before, the smallest such t on a tie. A hit is (start, end = t + 1, logp), best first. An end frame whose best
// window overlaps a taken one is dropped, even if a worse window ending there would not.
// cx: lane(), lanes(); any(b): b in some lane; best(v, t, s): the largest v over the lanes, the smallest t among equals, with
// its s, in every lane; put(j, s, e) / get(j, &s, &e): the j-th window taken (j < FIND_MAX_HITS). Every lane runs every
// call of cx together: the loops' bounds are the same in all of them.
template <class Ctx>
CTC_HD void find_select(Ctx& cx, const FindPhrase& ph, int max_hits, double min_logp) {
  const double NEG = align_neg_inf();
  const int T = ph.T, lane = cx.lane(), nl = cx.lanes();
  const double* const end_logp = ph.end_logp;
  const int32_t* const end_start = ph.end_start;
  int n = 0;
  for (; n < max_hits; ++n) {
    double bv = NEG;
    int bt = 0x7FFFFFFF, bs = -1;
    for (int t0 = 0; t0 < T; t0 += nl) {
      const int t = t0 + lane;
      const double v = t < T ? end_logp[t] : NEG;
      const int s = t < T ? end_start[t] : -1;
      // (a lane meets its frames in ascending order: an equal score keeps the smaller t)
      bool cand = v > NEG && v >= min_logp && v > bv;
      if (!cx.any(cand)) continue;
      for (int j = 0; j < n; ++j) {
        int hs, he;
        cx.get(j, &hs, &he);
        if (s < he && hs <= t) cand = false;
      }
      if (cand) bv = v, bt = t, bs = s;
    }
    cx.best(bv, bt, bs);
    if (bt == 0x7FFFFFFF) break;
    cx.put(n, bs, bt + 1);
    if (lane == 0) ph.hit_logp[n] = bv, ph.hit_start[n] = bs, ph.hit_end[n] = bt + 1;
  }
  if (lane == 0) *ph.n_hits = n;
}

// The trace's entry of frame t, by whoever owns state S - 2, the last label (entry jf = 1 or 3 of its group)
CTC_HD void find_trace(double* end_logp, int32_t* end_start, int t, int jf, const double* d, const int32_t* st) {
  const double v = jf == 1 ? d[1] : d[3];
  end_logp[t] = v;
  end_start[t] = v > align_neg_inf() ? (jf == 1 ? st[1] : st[3]) : -1;
}

// ctc_find: the threads of cx (tid, nt, sync(); Ctx::GROUPS * nt >= find_chunks(L)) share one phrase of a matrix of dtype DT,
// arranged as ctc_forward is: a group's scores and start frames stay in registers, and only its last state goes through `col`
// -- 2 * find_chunks(L) doubles, then as many int32: the columns of two successive frames -- to the thread that owns the group
// above: one barrier per frame. The thread that owns state S - 2 writes the trace; after the last frame its wavefront alone
// (cx.same_wave, after cx.publish) selects the hits from what it wrote.
template <int DT, class Ctx>
CTC_HD void ctc_find_phrase(Ctx& cx, const FindPhrase& ph, int V, int blank, double clip_lo, int max_hits, double min_logp, double* col) {
  constexpr int G = Ctx::GROUPS;
  double* const end_logp = ph.end_logp;  // (the record, once: the frame loop reads none of it again)
  int32_t* const end_start = ph.end_start;
  const int T = ph.T, L = ph.L;
  if (T <= 0 || L <= 0) return;
  const int nch = find_chunks(L);
  const int cf = (2 * L - 1) >> 2, jf = (2 * L - 1) & 3;  // state S - 2, the last label: entry 1 or 3 of its group
  const double NEG = align_neg_inf();
  double* const col_d = col;
  int32_t* const col_s = (int32_t*)(col + 2 * nch);
  ForwardGroup g[G];
  EntrySource<G> src;
  thread_setup(cx, ph.x, ph.lse, nullptr, ph.lab, L, nch, V, blank, ph.is_prob != 0, clip_lo, g, src);
  double d[G][4];    // scores
  int32_t st[G][4];  // start frames
  CTC_UNROLL
  for (int k = 0; k < G; ++k) {
    d[k][0] = d[k][1] = d[k][2] = d[k][3] = NEG;
    st[k][0] = st[k][1] = st[k][2] = st[k][3] = -1;
  }
  for (int i = cx.tid; i < 2 * nch; i += cx.nt) col_d[i] = NEG, col_s[i] = -1;
  cx.sync();
  FrameEntries<DT, G> now, next;
  now.request(src, 0);
  for (int t = 0; t < T; ++t) {
    const int po = ((t + 1) & 1) * nch, co = (t & 1) * nch;
    double dm1[G];
    int32_t sm1[G];
    CTC_UNROLL
    for (int k = 0; k < G; ++k) {
      const int c = cx.tid + k * cx.nt;
      dm1[k] = c > 0 && c < nch ? col_d[po + c - 1] : NEG;
      sm1[k] = c > 0 && c < nch ? col_s[po + c - 1] : -1;
    }
    next.request(src, t + 1 < T ? t + 1 : t);  // (after the last frame: the last frame again)
    const double e_blank = now.emit_blank(src);
    CTC_UNROLL
    for (int k = 0; k < G; ++k) {
      const int c = cx.tid + k * cx.nt;
      if (c >= nch) continue;
      find_step(g[k], c == 0, t, dm1[k], sm1[k], e_blank, now.emit0(src, k), now.emit1(src, k), d[k], st[k]);
      col_d[co + c] = d[k][3];
      col_s[co + c] = st[k][3];
      if (c == cf) find_trace(end_logp, end_start, t, jf, d[k], st[k]);
    }
    now = next;
    cx.sync();  // the one barrier of a frame: the columns swap roles
  }
  if (!cx.same_wave(cf % cx.nt)) return;
  cx.publish();
  find_select(cx, ph, max_hits, min_logp);
}

// ctc_find_wave: one wavefront per phrase of at most FIND_WAVE_MAX_LABELS labels. Lane c owns group c; the last state of the
// group below -- a score and a start frame -- comes from lane c - 1 by cx.up() / cx.up_i(): no LDS, no barrier. The same
// groups, steps and entries as ctc_find_phrase, so the same bits. Lane cf writes the trace, the wave selects.
template <int DT, class Ctx>
CTC_HD void ctc_find_wave_phrase(Ctx& cx, const FindPhrase& ph, int V, int blank, double clip_lo, int max_hits, double min_logp) {
  double* const end_logp = ph.end_logp;
  int32_t* const end_start = ph.end_start;
  const int T = ph.T, L = ph.L, c = cx.lane();
  if (T <= 0 || L <= 0) return;
  const int nch = find_chunks(L);
  const int cf = (2 * L - 1) >> 2, jf = (2 * L - 1) & 3;
  const double NEG = align_neg_inf();
  EntrySource<1> src = {ph.x, ph.lse, nullptr, V, blank, ph.is_prob != 0, clip_lo, {0}, {0}};
  const ForwardGroup g = group_setup(ph.lab, L, nch, c, blank, &src.i0[0], &src.i1[0]);
  double d[4] = {NEG, NEG, NEG, NEG};
  int32_t st[4] = {-1, -1, -1, -1};
  FrameEntries<DT, 1> now, next;
  now.request(src, 0);
  for (int t = 0; t < T; ++t) {
    const double below_d = cx.up(d[3]);  // (every lane takes part)
    const int32_t below_s = cx.up_i(st[3]);
    next.request(src, t + 1 < T ? t + 1 : t);
    if (c < nch) {
      find_step(g, c == 0, t, c > 0 ? below_d : NEG, c > 0 ? below_s : -1, now.emit_blank(src), now.emit0(src, 0), now.emit1(src, 0), d, st);
      if (c == cf) find_trace(end_logp, end_start, t, jf, d, st);
    }
    now = next;
  }
  cx.publish();
  find_select(cx, ph, max_hits, min_logp);
}

// ---- row_lse_max / ctc_viterbi_gaps ------------------------------------------------------------------------------------------
// Forced alignment of a target with gaps ("Alignment with gaps"). The states are ctc_viterbi's, S = 2L + 1: even
// state 2j is slot j (before label j; slot L follows the last label), odd state 2k + 1 is label k. A plain slot emits the
// blank; a gap slot emits g(t) = align_emit_of_value(largest entry of row t that is not a NaN, lse[t], ...): the best any
// label or the blank has in that frame, so the gap takes the frames nobody transcribed at the price the best unconstrained
// path would pay for them. Transitions are ctc_viterbi's. Equal scores prefer stay, then step, then skip in label states and
// plain slots; in a gap slot they prefer step over stay -- where a target label is its row's maximum, g(t) and the label's
// emission are the same bits, and this is the rule under which such a frame goes to the label at both of its ends.

// One row, one thread: row_lse_seq's blocks in row_lse_seq's order, and the running maximum that the sum was scaled by -- the
// largest entry that is not a NaN (-inf for a row without one). A probability-like row takes the maximum alone.
CTC_HD void row_lse_max_seq(const void* x, int dtype, size_t row0, int V, bool is_prob, double* lse_out, double* max_out) {
  if (is_prob) {
    double m = align_neg_inf();
    for (int i = 0; i < V; ++i) {
      const double v = align_load(x, dtype, row0 + (size_t)i);
      m = v > m ? v : m;
    }
    *max_out = m;
    return;
  }
  const LseAcc a = row_fold_seq(x, dtype, row0, V);
  *lse_out = lse_value(a);
  *max_out = a.m;
}

// One utterance of a ctc_viterbi_gaps launch. The host validates every field before a launch: the labels are in [0, V) and
// not the blank, L >= 1, T >= L + (adjacent equal labels), and every array is as long as its comment says.
struct GapsUtt {
  const void* x;        // [T, V] logits or probabilities, of the launch's dtype
  const double* lse;    // [T] log-sum-exp of each row (not read when is_prob)
  const double* rmax;   // [T] largest entry of each row that is not a NaN
  const int32_t* lab;   // [L] target labels
  const uint8_t* gap;   // [L + 1] 1: the slot is a gap
  uint8_t* bp;          // [T * align_chunks(L)] back-pointers, four 2-bit entries per byte
  int32_t* path;        // [T] out: the label taken at each frame, the blank id in a plain slot, -1 in a gap slot
  int32_t* tok_start;   // [L] out: first frame of each target label
  int32_t* tok_end;     // [L] out: one past its last frame
  double* tok_logp;     // [L] out (fold != 0): the fold of the label's log-probability over [tok_start, tok_end)
  double* gap_logp;     // [L + 1] out, gap slots only: the sum of g(t) over the slot's frames, in frame order
  double* score;        // [1] out: the sum of the log-probabilities along `path`
  int32_t T, L, is_prob, pad;
};

// One frame of one group (slot 2c, label 2c, slot 2c + 1, label 2c + 1: ForwardGroup), in place: p the group's scores at the
// frame before, pm1 that of the last state of the group below. gap0 / gap2: the group's two slots are gaps; e_gap = g(t).
// Returns the group's byte of back-pointers (0 stay, 1 step, 2 skip; state j in bits 2j, 2j + 1). Nothing but compares and
// additions -- ctc_viterbi's, operand for operand, where no slot is a gap: the same operands give the same bits wherever this
// is inlined.
CTC_HD unsigned gap_step(const ForwardGroup& g, bool gap0, bool gap2, double pm1, double e_blank, double e_gap, double e0, double e1,
                         double* p) {
  const double NEG = align_neg_inf();
  const double p0 = p[0], p1 = p[1], p2 = p[2], p3 = p[3];
  unsigned bp = 0;
  double b = p0;
  if (gap0 ? (pm1 >= b && pm1 > NEG) : pm1 > b) b = pm1, bp = 1u;
  p[0] = b + (gap0 ? e_gap : e_blank);
  if (g.l0 >= 0) {
    unsigned q = 0;
    b = p1;
    if (p0 > b) b = p0, q = 1u;
    if (g.skip0 && pm1 > b) b = pm1, q = 2u;
    bp |= q << 2;
    p[1] = b + e0;
  } else {
    p[1] = NEG;
  }
  if (g.blank2) {
    unsigned q = 0;
    b = p2;
    if (gap2 ? (p1 >= b && p1 > NEG) : p1 > b) b = p1, q = 1u;
    bp |= q << 4;
    p[2] = b + (gap2 ? e_gap : e_blank);
  } else {
    p[2] = NEG;
  }
  if (g.l1 >= 0) {
    unsigned q = 0;
    b = p3;
    if (p2 > b) b = p2, q = 1u;
    if (g.skip1 && p1 > b) b = p1, q = 2u;
    bp |= q << 6;
    p[3] = b + e1;
  } else {
    p[3] = NEG;
  }
  return bp;
}

// ctc_viterbi_gaps: the threads of cx (tid, nt, sync(); Ctx::GROUPS * nt >= align_chunks(L)) share one utterance of a matrix of
// dtype DT, arranged as ctc_forward / ctc_find are: a group's scores stay in registers, and only its last state goes through
// `col` -- 2 * align_chunks(L) doubles, the columns of two successive frames -- to the thread that owns the group above: one
// barrier per frame. A frame's entries are the blank, the group's labels, and the row's log-sum-exp and maximum. Per frame
// and group one byte of back-pointers, neighbouring threads writing neighbouring bytes. No window of reachable states: every
// state exists in every frame, and all but states 0 and 1 begin at -inf (every emission is finite, so -inf stays -inf until a
// path arrives; a state no path can leave towards the end is never traced). After the last frame the thread that owns the
// last state walks the back-pointers, as ctc_viterbi's does; then one thread per label folds its confidence and one thread per
// gap sums g(t) over the gap's frames.
template <int DT, class Ctx>
CTC_HD void ctc_viterbi_gaps_utt(Ctx& cx, const GapsUtt& utt, int V, int blank, int fold, double clip_lo, double* col) {
  constexpr int G = Ctx::GROUPS;
  const void* const x = utt.x;  // (the record, once: the frame loop reads none of it again)
  const double* const lse = utt.lse;
  const double* const rmax = utt.rmax;
  const int32_t* const lab = utt.lab;
  const uint8_t* const gap = utt.gap;
  uint8_t* const bps = utt.bp;
  const int T = utt.T, L = utt.L;
  const bool is_prob = utt.is_prob != 0;
  if (T <= 0 || L <= 0) return;
  const int S = 2 * L + 1, nch = align_chunks(L);
  const double NEG = align_neg_inf();
  ForwardGroup g[G];
  EntrySource<G> src;
  thread_setup(cx, x, is_prob ? rmax : lse, rmax, lab, L, nch, V, blank, is_prob, clip_lo, g, src);
  bool gap0[G], gap2[G];
  double p[G][4];  // scores
  CTC_UNROLL
  for (int k = 0; k < G; ++k) {
    const int c = cx.tid + k * cx.nt;
    p[k][0] = p[k][1] = p[k][2] = p[k][3] = NEG;
    gap0[k] = c < nch && 2 * c <= L && gap[2 * c] != 0;
    gap2[k] = c < nch && 2 * c + 1 <= L && gap[2 * c + 1] != 0;
  }
  for (int i = cx.tid; i < 2 * nch; i += cx.nt) col[i] = NEG;
  if (cx.tid == 0) {  // frame 0: states 0 and 1
    const double lse0 = is_prob ? 0.0 : lse[0];
    p[0][0] = gap0[0] ? align_emit_of_value(rmax[0], lse0, is_prob, clip_lo) : align_emit(x, DT, (size_t)blank, lse0, is_prob, clip_lo);
    p[0][1] = align_emit(x, DT, (size_t)lab[0], lse0, is_prob, clip_lo);
  }
  cx.sync();
  // frame 1's entries (a single frame: frame 0's again, never used)
  FrameEntries<DT, G, true> now, next;
  now.request(src, T > 1 ? 1 : 0);
  for (int t = 1; t < T; ++t) {
    const double* prev = col + ((t - 1) & 1) * nch;
    double* cur = col + (t & 1) * nch;
    double pm1[G];
    CTC_UNROLL
    for (int k = 0; k < G; ++k) {
      const int c = cx.tid + k * cx.nt;
      pm1[k] = c > 0 && c < nch ? prev[c - 1] : NEG;
    }
    next.request(src, t + 1 < T ? t + 1 : t);  // (after the last frame: the last frame again)
    const double e_blank = now.emit_blank(src), e_gap = now.emit_max(src);
    uint8_t* const bp_row = bps + (size_t)t * (size_t)nch;
    CTC_UNROLL
    for (int k = 0; k < G; ++k) {
      const int c = cx.tid + k * cx.nt;
      if (c >= nch) continue;
      const unsigned b = gap_step(g[k], gap0[k], gap2[k], pm1[k], e_blank, e_gap, now.emit0(src, k), now.emit1(src, k), p[k]);
      cur[c] = p[k][3];
      bp_row[c] = (uint8_t)b;
    }
    now = next;
    cx.sync();  // the one barrier of a frame: the columns swap roles
  }
  // back-trace, by the thread that holds the last slot (state S - 1 = 2L: entry 0 or 2 of its group; the last label is the
  // entry before it). The last label is preferred over the trailing slot.
  const int cf = (S - 1) >> 2, jf = (S - 1) & 3;
  const double* fin = col + ((T - 1) & 1) * nch;
  CTC_UNROLL
  for (int k = 0; k < G; ++k) {
    if (cx.tid + k * cx.nt != cf) continue;
    const double last = jf == 2 ? p[k][2] : p[k][0];
    const double before = jf == 2 ? p[k][1] : fin[cf - 1];  // (L >= 1: jf == 0 only in a group above the first)
    *utt.score = before >= last ? before : last;
    viterbi_backtrace(before >= last ? S - 2 : S - 1, T, nch, bps, lab, utt.path, utt.tok_start, utt.tok_end,
                      [&](int j) { return gap[j] ? -1 : blank; });
  }
  cx.sync();  // (the spans that thread wrote are read by every thread)
  for (int j = cx.tid; j <= L; j += cx.nt) {
    if (!gap[j]) continue;
    int t0 = j > 0 ? utt.tok_end[j - 1] : 0, t1 = j < L ? utt.tok_start[j] : T;
    t0 = t0 < 0 ? 0 : t0;
    t1 = t1 > T ? T : t1;
    double acc = 0.0;
    for (int t = t0; t < t1; ++t) acc += align_emit_of_value(rmax[t], is_prob ? 0.0 : lse[t], is_prob, clip_lo);
    utt.gap_logp[j] = acc;
  }
  if (fold) fold_token_logp(cx, x, DT, lse, lab, utt.tok_start, utt.tok_end, utt.tok_logp, T, L, V, is_prob, fold, clip_lo);
}

// ---- row_argmax / row_lse_argmax / greedy_collapse ---------------------------------------------------------------------------
// Greedy best-path decoding ("Greedy decode"): every frame takes its most probable label, runs of one label are one
// token, blanks separate tokens and are dropped.

// What a lane knows of a row: its largest entry that is not a NaN and the smallest index that holds it (ARG_NONE: no entry
// above -inf so far). Two of them merge by (value, index), so the result does not depend on which lane folded which entry.
constexpr int32_t ARG_NONE = 0x7FFFFFFF;
template <class VT>
CTC_HD void arg_merge(VT& v, int32_t& i, VT ov, int32_t oi) {
  if (ov > v || (ov == v && oi < i)) v = ov, i = oi;
}

// One row, one thread (the simulator): the smallest index among the entries equal to the row's largest entry that is not a
// NaN; the blank for a row without an entry above -inf. Compares alone: -0.0 and +0.0 are equal, a NaN is never greater.
CTC_HD int32_t row_argmax_seq(const void* x, int dtype, size_t row0, int V, int blank) {
  double m = align_neg_inf();
  int32_t arg = ARG_NONE;
  for (int i = 0; i < V; ++i) {
    const double v = align_load(x, dtype, row0 + (size_t)i);
    if (v > m) m = v, arg = i;
  }
  return arg == ARG_NONE ? blank : arg;
}

// One greedy_collapse launch: utterance u's frame labels are arg[row0[u] .. row0[u + 1]). The count pass (write == 0) leaves
// the utterance's number of tokens in count[u]; the host scans the counts into tok_off, and the write pass puts token k of
// utterance u at tok_off[u] + k of label / start / end -- compact across the batch. With a fold the write pass also sums
// e(t) = align_emit_of_value(rmax[t], lse[t], ...) over all frames into score[u] and folds it over each token's frames.
struct GreedyArgs {
  const int32_t* arg;        // [n_rows] every row's label
  const int64_t* row0;       // [n_utts + 1]
  const int64_t* tok_off;    // [n_utts + 1] (write pass)
  int32_t* count;            // [n_utts] out (count pass)
  int32_t* label;            // [n_tokens] out (write pass), like start and end
  int32_t* start;
  int32_t* end;              // one past the token's last frame
  const double* lse;         // [n_rows] (fold) row log-sum-exps of the logit utterances
  const double* rmax;        // [n_rows] (fold) every row's largest entry that is not a NaN
  const uint32_t* is_prob;   // [n_utts] (fold)
  double* logp;              // [n_tokens] out (fold)
  double* score;             // [n_utts] out (fold)
  int32_t n_utts, blank, fold, write;
  double clip_lo;
};

// One utterance by the lanes of cx, which take lanes() frames a step, lane l the frame t0 + l: lane(), lanes(), up(v) / down(v)
// (the neighbour lane's v; the lane's own at the edge), first(v) / last(v) (the first / last lane's v), ballot(b) (bit l: lane
// l's b) and publish() (this wave's stores, visible to its loads). A frame past the end reads as a blank, like the frame
// before the first. A run starts where the label is no blank and differs from the frame before, and ends where it differs
// from the frame after: the ballots of both give each token's ordinal by a count of the bits below the lane's.
CTC_HD int32_t greedy_popcount(uint64_t bits) { return (int32_t)__builtin_popcountll(bits); }
template <class Ctx>
CTC_HD void greedy_collapse_utt(Ctx& cx, const GreedyArgs& a, int u) {
  const int64_t r0 = a.row0[u];
  const int T = (int)(a.row0[u + 1] - r0);
  const int32_t* arg = a.arg + r0;
  const int W = cx.lanes(), lane = cx.lane(), blank = a.blank;
  const bool write = a.write != 0;
  const int64_t o = write ? a.tok_off[u] : 0;
  const uint64_t below = ((uint64_t)1 << lane) - 1;
  int32_t n_start = 0, n_end = 0;
  int32_t before = blank;  // the label of the frame before the step's first
  int32_t cur = lane < T ? arg[lane] : blank;
  for (int t0 = 0; t0 < T; t0 += W) {
    const int t = t0 + lane;
    const int32_t next = (int64_t)t + W < T ? arg[t + W] : blank;  // (the step after this one)
    int32_t left = cx.up(cur), right = cx.down(cur);
    const int32_t after = cx.first(next);
    if (lane == 0) left = before;
    if (lane == W - 1) right = after;
    const bool starts = cur != blank && cur != left, ends = cur != blank && cur != right;
    const uint64_t bs = cx.ballot(starts), be = cx.ballot(ends);
    if (write && starts) {
      const int64_t k = o + n_start + greedy_popcount(bs & below);
      a.label[k] = cur;
      a.start[k] = t;
    }
    if (write && ends) a.end[o + n_end + greedy_popcount(be & below)] = t + 1;
    n_start += greedy_popcount(bs);
    n_end += greedy_popcount(be);
    before = cx.last(cur);
    cur = next;
  }
  if (!write) {
    if (lane == 0) a.count[u] = n_start;
    return;
  }
  if (!a.fold) return;
  cx.publish();  // (the spans: stored by the lanes that met them, loaded by the lanes the tokens are dealt to)
  const bool is_prob = a.is_prob[u] != 0;
  const double* lse = a.lse + r0;
  const double* rmax = a.rmax + r0;
  const auto e = [&](int t) { return align_emit_of_value(rmax[t], is_prob ? 0.0 : lse[t], is_prob, a.clip_lo); };
  if (lane == 0) {  // in frame order, as ctc_viterbi adds a path's frames
    double acc = 0.0;
    for (int t = 0; t < T; ++t) acc = t == 0 ? e(0) : acc + e(t);
    a.score[u] = acc;
  }
  for (int k = lane; k < n_start; k += W) {  // fold_token_logp's fold, of e(t)
    int t0 = a.start[o + k], t1 = a.end[o + k];
    t0 = t0 < 0 ? 0 : t0;
    t1 = t1 > T ? T : t1;
    double acc = 0.0;
    for (int t = t0; t < t1; ++t) {
      const double lp = e(t);
      if (a.fold == LOGP_MEAN) acc += lp;
      else if (a.fold == LOGP_MIN) acc = (t == t0 || lp < acc) ? lp : acc;
      else acc = (t == t0 || lp > acc) ? lp : acc;
    }
    a.logp[o + k] = a.fold == LOGP_MEAN ? acc / (double)(t1 - t0) : acc;
  }
}

// ---- ctc_prefix_extend -------------------------------------------------------------------------------------------------------
// The CTC prefix score ("Prefix scores"): for a prefix g of L labels and every label c at once,
//   next(g)[c] = log sum_t exp(W_c[t] + e(t, c)),   W_c = B if c is g's last label, else A,
//   B[t] = a_{t-1}[S-1],  A[t] = lse2(a_{t-1}[S-1], a_{t-1}[S-2])   (PrefixEnds: the forward bodies store both addends),
// as a scaled product instead of a log-sum-exp per element: with m = PrefixEnds::scale (max_t A[t] - ln 2 <= m <= max_t A[t]),
//   wB[t] = exp(bc[t] - m),  wA[t] = wB[t] + exp(bc[T + t] - m)   (A is never formed: its weight is the sum of two),
//   next(g)[c] = m + log( sum_t w_c[t] * exp(e(t, c)) ),   -inf for an empty sum and for the blank.
// exp(e) lies in [1e-15, 1] and is formed once per entry for all the prefixes of a chunk; a weight more than about 700 below
// m is 0, which changes a sum by less than e^-650 of itself. The frames are cut into segments of PREFIX_SEG; a segment's
// sum runs in frame order from 0.0 by fma, the segments' sums are added in ascending order from 0.0 -- inside one workgroup
// or, when the launch is split, by ctc_prefix_finish from `partial`: the same additions either way, so the same bits.
constexpr int32_t PREFIX_K = 8;       // prefixes of one utterance that share a read of its rows: 2 K accumulator registers a thread
constexpr int32_t PREFIX_SEG = 128;   // frames of a segment
constexpr int32_t PREFIX_COLS = 256;  // columns of a tile: one to a thread
constexpr int32_t PREFIX_W_DOUBLES = (2 * PREFIX_K + 1) * PREFIX_SEG;  // a segment's weights (A's and B's per prefix) and log-sum-exps
constexpr int32_t PREFIX_FUSE_BLOCKS = 1024;  // a launch with fewer (chunk, tile) pairs is split by segments as well

// Up to PREFIX_K prefixes of one utterance. The host validates every field before a launch.
struct PrefixChunk {
  const void* x;        // [T, V] the utterance's matrix, of the launch's dtype
  const double* lse;    // [T] log-sum-exp of each row (not read when is_prob)
  int32_t h[PREFIX_K];  // the prefixes, as indices of the call ([0, n) used)
  int32_t n, T, is_prob, pad;
};
struct PrefixExtendArgs {
  const PrefixChunk* chunks;  // [n_chunks] (device)
  const PrefixEnds* ends;     // [prefixes of the call] (device): what the forward pass stored; read for the chunks' prefixes only
  const int32_t* last;        // [prefixes of the call] (device): a prefix's last label, -1 for the empty one
  double* next;               // [prefixes of the call][V] out
  double* partial;            // (split) [n_chunks][max_segs][PREFIX_K][V] the segments' sums
  int32_t n_chunks, n_labels, dtype, blank;
  int32_t max_segs;           // the most segments an utterance of the launch has
  int32_t split;              // 1: a workgroup takes one segment and stores its sums; 0: all of them, and stores the result
  double clip_lo;             // ln(MIN_TOKEN_CLIP_P)
};
CTC_HD int32_t prefix_segments(int32_t T) { return (T + PREFIX_SEG - 1) / PREFIX_SEG; }
CTC_HD int32_t prefix_tiles(int32_t V) { return (V + PREFIX_COLS - 1) / PREFIX_COLS; }
// (host) the one rule for `split`: by the launch's size alone; the result's bits do not depend on it
inline bool prefix_split(int64_t n_chunks, int32_t V) { return n_chunks * (int64_t)prefix_tiles(V) < PREFIX_FUSE_BLOCKS; }
CTC_HD size_t prefix_partial_at(const PrefixExtendArgs& a, int chunk, int seg, int k, int c) {
  return (((size_t)chunk * (size_t)a.max_segs + (size_t)seg) * PREFIX_K + (size_t)k) * (size_t)a.n_labels + (size_t)c;
}

// A segment's weights, by all threads of cx: w[(2 k) * SEG + j] = wA, w[(2 k + 1) * SEG + j] = wB of prefix k at frame
// seg * SEG + j (0 past the chunk's prefixes and past T), w[2 K * SEG + j] the row's log-sum-exp (0 where none is read)
template <class Ctx>
CTC_HD void prefix_weights(Ctx& cx, const PrefixExtendArgs& a, const PrefixChunk& ch, int seg, double* w) {
  const double NEG = align_neg_inf();
  const int T = ch.T, t0 = seg * PREFIX_SEG;
  for (int i = cx.tid; i < PREFIX_K * PREFIX_SEG; i += cx.nt) {
    const int k = i / PREFIX_SEG, j = i % PREFIX_SEG, t = t0 + j;
    double wa = 0.0, wb = 0.0;
    if (k < ch.n && t < T) {
      const PrefixEnds e = a.ends[ch.h[k]];
      const double m = *e.scale, b = e.bc[t], c = e.bc[T + t];
      wb = b > NEG ? exp(b - m) : 0.0;  // (an end state above -inf: m is finite and not below it)
      wa = wb + (c > NEG ? exp(c - m) : 0.0);
    }
    w[(2 * k) * PREFIX_SEG + j] = wa;
    w[(2 * k + 1) * PREFIX_SEG + j] = wb;
  }
  for (int j = cx.tid; j < PREFIX_SEG; j += cx.nt) w[2 * PREFIX_K * PREFIX_SEG + j] = !ch.is_prob && t0 + j < T ? ch.lse[t0 + j] : 0.0;
}

// exp(e(t, c)) of an entry as loaded: the clipped probability itself, or exp of the clipped x - lse. A NaN takes the floor.
CTC_HD double prefix_exp_emit(double v, double lse, bool is_prob, double clip_lo) {
  if (is_prob) return !(v >= 1e-15) ? 1e-15 : (v > 1.0 ? 1.0 : v);
  const double y = v - lse;
  return exp(!(y >= clip_lo) ? clip_lo : (y > 0.0 ? 0.0 : y));
}

// Column c's sums over the nf frames of one segment, from 0.0 in frame order: acc[k] for the chunk's n prefixes, whose
// weights start at w[base[k]] (FULL: n == PREFIX_K, no test per prefix). Four rows are asked for ahead of their use.
template <int DT, bool FULL>
CTC_HD void prefix_fold_segment(const void* x, int V, int c, int t0, int nf, bool is_prob, double clip_lo, int n, const double* w,
                                const int* base, double* acc) {
  typedef typename AlignRaw<DT>::type Raw;
  const double* lse_w = w + 2 * PREFIX_K * PREFIX_SEG;
  for (int j = 0; j < nf; j += 4) {
    Raw r[4];
    CTC_UNROLL
    for (int i = 0; i < 4; ++i) {
      const int jj = j + i < nf ? j + i : nf - 1;
      r[i] = align_load_raw<DT>(x, (size_t)(t0 + jj) * (size_t)V + (size_t)c);
    }
    CTC_UNROLL
    for (int i = 0; i < 4; ++i) {
      if (j + i >= nf) break;
      const double ee = prefix_exp_emit(align_widen<DT>(r[i]), lse_w[j + i], is_prob, clip_lo);
      CTC_UNROLL
      for (int k = 0; k < PREFIX_K; ++k)
        if (FULL || k < n) acc[k] = fma(w[base[k] + j + i], ee, acc[k]);
    }
  }
}

CTC_HD void prefix_store(const PrefixExtendArgs& a, int h, int c, double total) {
  a.next[(size_t)h * (size_t)a.n_labels + (size_t)c] = (c == a.blank || !(total > 0.0)) ? align_neg_inf() : *a.ends[h].scale + log(total);
}

// The threads of cx (tid, nt, sync()) share the segments [s0, s1) of one chunk; this thread owns column c (any c >= V: it
// only helps with the weights). `w`: PREFIX_W_DOUBLES doubles shared by the threads. Every thread of cx makes the call with
// the same chunk, s0 and s1.
template <int DT, class Ctx>
CTC_HD void ctc_prefix_extend_tile(Ctx& cx, const PrefixExtendArgs& a, int chunk, int c, int s0, int s1, double* w) {
  const PrefixChunk& ch = a.chunks[chunk];
  const int T = ch.T, V = a.n_labels, n = ch.n;
  const bool live = c < V, is_prob = ch.is_prob != 0;
  int base[PREFIX_K];  // the column of the prefix' last label takes B's weights: a choice of row, made once
  double total[PREFIX_K];
  CTC_UNROLL
  for (int k = 0; k < PREFIX_K; ++k) {
    base[k] = (2 * k + (live && k < n && a.last[ch.h[k]] == c ? 1 : 0)) * PREFIX_SEG;
    total[k] = 0.0;
  }
  for (int seg = s0; seg < s1; ++seg) {
    cx.sync();  // (the weights of the segment before are done with)
    prefix_weights(cx, a, ch, seg, w);
    cx.sync();
    if (!live) continue;
    const int t0 = seg * PREFIX_SEG, nf = T - t0 < PREFIX_SEG ? T - t0 : PREFIX_SEG;
    double acc[PREFIX_K];
    CTC_UNROLL
    for (int k = 0; k < PREFIX_K; ++k) acc[k] = 0.0;
    if (n == PREFIX_K) prefix_fold_segment<DT, true>(ch.x, V, c, t0, nf, is_prob, a.clip_lo, n, w, base, acc);
    else prefix_fold_segment<DT, false>(ch.x, V, c, t0, nf, is_prob, a.clip_lo, n, w, base, acc);
    CTC_UNROLL
    for (int k = 0; k < PREFIX_K; ++k) {
      if (k >= n) continue;
      if (a.split) a.partial[prefix_partial_at(a, chunk, seg, k, c)] = acc[k];
      else total[k] += acc[k];
    }
  }
  if (a.split || !live) return;
  CTC_UNROLL
  for (int k = 0; k < PREFIX_K; ++k)
    if (k < n) prefix_store(a, ch.h[k], c, total[k]);
}

// (split) column c of one chunk: the segments' sums in ascending order, as ctc_prefix_extend_tile adds its own
CTC_HD void ctc_prefix_finish_col(const PrefixExtendArgs& a, int chunk, int c) {
  const PrefixChunk& ch = a.chunks[chunk];
  const int nseg = prefix_segments(ch.T);
  for (int k = 0; k < ch.n; ++k) {
    double total = 0.0;
    for (int seg = 0; seg < nseg; ++seg) total += a.partial[prefix_partial_at(a, chunk, seg, k, c)];
    prefix_store(a, ch.h[k], c, total);
  }
}

// ---- ctc_prefix_advance ------------------------------------------------------------------------------------------------------
// A prefix session ("Prefix sessions"): the PrefixEnds of the child g + [c] from the PrefixEnds of its parent g,
// without g's other states. Of the child's S = 2 (L + 1) + 1 states only the last label, y = a[S-2], and the final blank,
// z = a[S-1], are new; what feeds them from below is g's final blank and g's last label, which g's bc holds frame by frame:
//   y_0 = e(0, c) for the empty g, else -inf;  z_0 = -inf;
//   y_t = lse3(y_{t-1}, bc_g[t], c != last(g) ? bc_g[T + t] : -inf) + e(t, c),   z_t = lse2(z_{t-1}, y_{t-1}) + e(t, blank),
//   bc[t] = z_{t-1},  bc[T + t] = y_{t-1},  scale = their running maximum,  end = lse2(z_{T-1}, y_{T-1}).
// These are forward_step's calls for the child's last group -- the same functions on the same operands in the same order --
// and forward_window never withholds an operand: its lower edge stays below S - 4 until the last frame, and a state above
// its upper edge is -inf under the recursion as well. So the child's bc, scale and end are, bit for bit, what the forward
// bodies with ENDS store for g + [c]. One child of a launch; the host validates every field before it.
struct PrefixChild {
  const void* x;         // [T, V] the utterance's matrix, of the launch's dtype
  const double* lse;     // [T] log-sum-exp of each row (read, not used, when is_prob)
  const double* parent;  // [2 T] the parent's bc
  double* bc;            // [2 T] out
  double* scale;         // [1] out
  double* end;           // [1] out
  int32_t T, c, parent_last, is_prob;  // parent_last: -1 for the empty prefix
};
struct PrefixAdvanceArgs {
  const PrefixChild* kids;  // [n_kids] (device), the children of one utterance next to each other
  int32_t n_kids, n_labels, dtype, blank;
  double clip_lo;           // ln(MIN_TOKEN_CLIP_P)
};
constexpr int32_t PREFIX_ADVANCE_THREADS = 64;  // children of a workgroup: one wavefront
constexpr int32_t PREFIX_ADVANCE_AHEAD = 4;     // frames whose operands are asked for ahead of their use

// The operands of PREFIX_ADVANCE_AHEAD consecutive frames, kept as loaded. None of their addresses depends on the recursion.
template <int DT>
struct AdvanceFrames {
  typedef typename AlignRaw<DT>::type Raw;
  Raw vc[PREFIX_ADVANCE_AHEAD], vb[PREFIX_ADVANCE_AHEAD];
  double lse_t[PREFIX_ADVANCE_AHEAD], pb[PREFIX_ADVANCE_AHEAD], pl[PREFIX_ADVANCE_AHEAD];
  // frames t0 .. t0 + AHEAD - 1, those past the last frame the last frame again: loads alone, at indices that are always valid
  CTC_HD void request(const PrefixChild& k, int V, int blank, int t0) {
    CTC_UNROLL
    for (int i = 0; i < PREFIX_ADVANCE_AHEAD; ++i) {
      const int t = t0 + i < k.T ? t0 + i : k.T - 1;
      const size_t row = (size_t)t * (size_t)V;
      vc[i] = align_load_raw<DT>(k.x, row + (size_t)k.c);
      vb[i] = align_load_raw<DT>(k.x, row + (size_t)blank);
      lse_t[i] = k.lse[t];
      pb[i] = k.parent[t];
      pl[i] = k.parent[(size_t)k.T + (size_t)t];
    }
  }
};

template <int DT>
CTC_HD void ctc_prefix_advance_child(const PrefixChild& k, int V, int blank, double clip_lo) {
  const int T = k.T;
  if (T <= 0) return;
  const double NEG = align_neg_inf();
  const bool is_prob = k.is_prob != 0, skip = k.parent_last >= 0 && k.parent_last != k.c;
  double* const bc = k.bc;
  double y = k.parent_last < 0 ? align_emit(k.x, DT, (size_t)k.c, is_prob ? 0.0 : k.lse[0], is_prob, clip_lo) : NEG;
  double z = NEG, ends_m = NEG;
  bc[0] = NEG, bc[T] = NEG;
  AdvanceFrames<DT> cur, nxt;
  nxt.request(k, V, blank, 1);
  for (int t0 = 1; t0 < T; t0 += PREFIX_ADVANCE_AHEAD) {
    cur = nxt;
    nxt.request(k, V, blank, t0 + PREFIX_ADVANCE_AHEAD);
    CTC_UNROLL
    for (int i = 0; i < PREFIX_ADVANCE_AHEAD; ++i) {
      const int t = t0 + i;
      if (t >= T) break;
      bc[t] = z;
      bc[(size_t)T + (size_t)t] = y;
      ends_m = z > ends_m ? z : ends_m;
      ends_m = y > ends_m ? y : ends_m;
      const double lse_use = is_prob ? 0.0 : cur.lse_t[i];
      const double e_blank = align_emit_of_value(align_widen<DT>(cur.vb[i]), lse_use, is_prob, clip_lo);
      const double e_c = align_emit_of_value(align_widen<DT>(cur.vc[i]), lse_use, is_prob, clip_lo);
      const double y1 = align_lse3(y, cur.pb[i], skip ? cur.pl[i] : NEG) + e_c;
      z = align_lse2(z, y) + e_blank;
      y = y1;
    }
  }
  *k.end = align_lse2(z, y);
  *k.scale = ends_m;
}

}  // namespace ctc
