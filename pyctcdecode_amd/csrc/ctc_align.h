// ctc_align.h -- forced alignment of a known label sequence to an utterance's frames ("Forced alignment"): the
// fp64 log-sum-exp of a frame row and the Viterbi recursion over the blank / label / blank / ... states, with its back-trace
// and the confidence fold over the path. One body each for the HIP kernels (ctc_align_hip.hip: row_lse, ctc_viterbi) and for
// the CPU simulator build, whose "device" memory is host memory (api.cpp under CTC_SIM runs them with a one-thread context).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

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
CTC_HD double align_emit(const void* x, int dtype, size_t i, double lse, bool is_prob, double clip_lo) {
  const double v = align_load(x, dtype, i);
  if (is_prob) return log(!(v >= 1e-15) ? 1e-15 : (v > 1.0 ? 1.0 : v));
  const double y = v - lse;
  return !(y >= clip_lo) ? clip_lo : (y > 0.0 ? 0.0 : y);
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
CTC_HD double row_lse_seq(const void* x, int dtype, size_t row0, int V) {
  LseAcc a = lse_empty();
  double v[ALIGN_LSE_BLOCK];
  for (int b = 0; b < V; b += ALIGN_LSE_BLOCK) {
    for (int i = 0; i < ALIGN_LSE_BLOCK; ++i) v[i] = b + i < V ? align_load(x, dtype, row0 + (size_t)(b + i)) : align_neg_inf();
    lse_push_block(a, v);
  }
  return lse_value(a);
}

// ---- ctc_viterbi -------------------------------------------------------------------------------------------------------------
// State s of the 2L+1: even = a blank, odd = target label s >> 1. A thread owns groups of four consecutive states (blank,
// label 2c, blank, label 2c + 1), reads the previous column of scores from `col`, writes the current one and one byte of four
// back-pointers (0 stay, 1 step, 2 skip). Equal scores prefer stay, then step, then skip. Frame t only works on the groups
// that hold a state reachable from the start (s <= 2t + 1) and from the end (s >= S - 2 - 2(T - 1 - t)); what lies below the
// window of the previous frame reads as unreachable. `col`: 2 * 4 * align_chunks(L) doubles, shared by the threads of cx.
// cx: tid, nt, sync().
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
    int open = -1;
    for (int t = T - 1; t >= 0; --t) {
      if (s & 1) {
        const int k = s >> 1;
        if (k != open) u.tok_end[k] = t + 1, open = k;
        u.tok_start[k] = t;
        u.path[t] = u.lab[k];
      } else {
        u.path[t] = blank;
      }
      if (t > 0) {
        const unsigned b = (u.bp[(size_t)t * (size_t)nch + (size_t)(s >> 2)] >> (2 * (s & 3))) & 3u;
        s -= (int)b;
        if (s < 0) s = 0;
      }
    }
  }
  if (!fold) return;
  cx.sync();  // (the spans thread 0 wrote are read by every thread)
  for (int k = cx.tid; k < L; k += cx.nt) {
    int t0 = u.tok_start[k], t1 = u.tok_end[k];
    t0 = t0 < 0 ? 0 : t0;
    t1 = t1 > T ? T : t1;
    const size_t lab = (size_t)u.lab[k];
    double acc = 0.0;
    for (int t = t0; t < t1; ++t) {
      const double lp = align_emit(u.x, dtype, (size_t)t * (size_t)V + lab, is_prob ? 0.0 : u.lse[t], is_prob, clip_lo);
      if (fold == LOGP_MEAN) acc += lp;
      else if (fold == LOGP_MIN) acc = (t == t0 || lp < acc) ? lp : acc;
      else acc = (t == t0 || lp > acc) ? lp : acc;
    }
    u.tok_logp[k] = fold == LOGP_MEAN ? acc / (double)(t1 - t0) : acc;
  }
}

}  // namespace ctc
