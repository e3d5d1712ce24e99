// frame_prune_hip.hip -- the frame-prune stage on gfx950 (MI355X, CDNA4, wave64), in a translation unit of its own: the stage
// that streams the [T x V] logits from HBM exactly once and leaves every frame's surviving labels for the beam stage.
//
//   frame_prune<T>, frame_prune_f32x4<NC, PK>   one wave per frame row: log-softmax + clip (decoder.py:180-197,762-765), token
//                                               prune and argmax (decoder.py:444-445), the survivors in CPython-set order
//                                               (set_order.h; up to 18 keys in registers: wave_set_order), the row sum for
//                                               the input sniff. <T>: any dtype, label count and alignment; f32x4: float32
//                                               rows of up to 1024 labels in 16-byte loads, the row in registers
//   frame_prune_fast<NC, DT, AL, NP>            64 rows per wave in two phases (see there): the hot kernel. float32 rows of up
//                                               to 4095 labels, float16 / bfloat16 rows of up to 1024; NP: the reference's own
//                                               float32 arithmetic (np_f32.h, np_sum.h; NpPlan is numpy's summation order)
//   frame_prune[_f32x4]_listed                  the per-row code on the rows frame_prune_fast hands over (PruneArgs::slow_rows)
//   utt_sniff, utt_recount, utt_sniff_exact     decoder.py:760 (mean row sum ~ 1 => probabilities: those utterances get a
//                                               second pass with log(clip(p))) and the survivor count of the whole launch
//
// Which kernel a call takes: prune_route.h, a host-only function of the call's shape. launch_prune_on sets the call up and
// launches what the route names on the stream it is given; the stream and the timing events belong to backend_hip.hip.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <algorithm>
#include <type_traits>
#include <vector>
#include <math.h>
#include <stdlib.h>

#include "backend.h"
#include "set_order.h"
#include "np_f32.h"
#include "set_order_small.h"
#include "np_sum.h"
#include "wave_ops_hip.h"
#include "hip_try.h"
#include "prune_route.h"

namespace ctc {
namespace be {

template <typename T>
__device__ __forceinline__ double ld(const T* p, size_t i) {
  return (double)p[i];
}
// 16-bit logits straight from the acoustic model: exact widening to fp64 (no intermediate fp32 copy)
struct half_bits { uint16_t u; };
struct bf16_bits { uint16_t u; };
template <>
__device__ __forceinline__ double ld<half_bits>(const half_bits* p, size_t i) {
  return (double)__half2float(__ushort_as_half(p[i].u));
}
template <>
__device__ __forceinline__ double ld<bf16_bits>(const bf16_bits* p, size_t i) {
  return (double)__uint_as_float(((uint32_t)p[i].u) << 16);
}

// row -> utterance (binary search over the prefix sums)
__device__ __forceinline__ int find_utt(const int64_t* row0, int n_utts, int64_t row) {
  int lo = 0, hi = n_utts - 1;
  while (lo < hi) {
    int mid = (lo + hi + 1) >> 1;
    if (row0[mid] <= row) lo = mid; else hi = mid - 1;
  }
  return lo;
}

constexpr int PRUNE_WAVES = 4;  // rows per 256-thread block

// decoder.py:760 in two steps. The reference tests  math.isclose(logits.sum(axis=1).mean(), 1)  in the INPUT dtype, and for
// float32 / float16 that is in effect "does numpy's mean round to exactly 1". The frame-prune pass leaves exact (fp64) row
// sums; an utterance whose fp64 mean is nowhere near 1 is not a probability matrix in any summation order, everything
// else is marked ambiguous (2) and settled by utt_sniff_exact in numpy's own order and precision (np_sum.h).
__global__ __launch_bounds__(64) void utt_sniff(PruneArgs a) {
  const int u = blockIdx.x;
  const int lane = threadIdx.x;
  const int64_t r0 = a.utt_row0[u], r1 = a.utt_row0[u + 1];
  double s = 0.0, c = 0.0;
  {  // four rows per lane and trip: the loads of a trip are in flight together (one row per trip: 58 us of load latency for 4096 x 1000 rows)
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
    uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    for (int64_t r = r0 + lane; r < r1; r += 256) {
      const bool h1 = r + 64 < r1, h2 = r + 128 < r1, h3 = r + 192 < r1;
      const double x0 = a.row_sum[r], x1 = h1 ? a.row_sum[r + 64] : 0.0, x2 = h2 ? a.row_sum[r + 128] : 0.0, x3 = h3 ? a.row_sum[r + 192] : 0.0;
      const uint32_t n0 = a.surv_cnt[r], n1 = h1 ? a.surv_cnt[r + 64] : 0u, n2 = h2 ? a.surv_cnt[r + 128] : 0u, n3 = h3 ? a.surv_cnt[r + 192] : 0u;
      s += x0; s1 += x1; s2 += x2; s3 += x3;
      c0 += n0; c1 += n1; c2 += n2; c3 += n3;
    }
    s = (s + s1) + (s2 + s3);
    c = (double)c0 + (double)c1 + (double)c2 + (double)c3;
  }
  s = wave_sum(s);
  c = wave_sum(c);
  if (lane == 0) {
    // (the survivors of all rows, summed: what a small batch's beam kernel is chosen by; saturating, only read for small batches)
    // (only small batches read it, and 4096 atomics on one address are 40 us of a 55-us kernel: launches of more than 1024
    //  utterances leave it alone)
    if (a.pass == 0 && a.n_utts <= 1024) atomicAdd(&a.overflow[4], (uint32_t)fmin(c, 1.0e9));
    double mean = r1 > r0 ? s / (double)(r1 - r0) : NAN;
    // (an infinite mean -- rows masked with -inf -- is never close: math.isclose(+-inf, 1) is False.) The window:
    // float32 pairwise sums of rows of ordinary logits are off by < 1e-2; float64 ones by < 1e-12.
    const bool amb = isfinite(mean) && fabs(mean - 1.0) <= (a.dtype == 1 ? 1e-6 : 0.5);
    // (time-sliced ingest: the reference tests the WHOLE utterance's mean row sum -- the slices' sums are added up for the caller)
    if (a.utt_sum && r1 > r0) atomicAdd(&a.utt_sum[u], s);
    a.utt_is_prob[u] = amb ? 2u : 0u;
    if (amb) a.overflow[2] = 1u;  // flags[2]: some utterance needs the exact test
  }
}
// pass 1 redid the rows of the probability utterances as log(clip(p)): the survivors of all rows counted again (pass 0 counted
// those rows as logits -- softmax outputs read as logits are nearly flat, almost every label survives -- and a small batch
// chooses its beam kernel by this number). The caller zeroes overflow[4] before the pass.
__global__ __launch_bounds__(64) void utt_recount(PruneArgs a) {
  const int u = blockIdx.x;
  const int lane = threadIdx.x;
  const int64_t r0 = a.utt_row0[u], r1 = a.utt_row0[u + 1];
  double c = 0.0;
  for (int64_t r = r0 + lane; r < r1; r += 64) c += (double)a.surv_cnt[r];
  c = wave_sum(c);
  if (lane == 0) atomicAdd(&a.overflow[4], (uint32_t)fmin(c, 1.0e9));
}
// one workgroup per ambiguous utterance, one thread per row (rare path: probability inputs, or logits whose rows sum to ~1)
__global__ __launch_bounds__(256) void utt_sniff_exact(PruneArgs a) {
  const int u = blockIdx.x;
  if (a.utt_is_prob[u] != 2u) return;
  const int64_t r0 = a.utt_row0[u], T = a.utt_row0[u + 1] - r0;
  const void* x = a.utt_logits[u];
  for (int64_t t = threadIdx.x; t < T; t += blockDim.x) a.row_sum[r0 + t] = np_row_sum(x, a.dtype, t, a.n_labels);
  __syncthreads();
  if (threadIdx.x == 0) {
    const bool is_prob = T > 0 && np_mean_is_one(np_mean_of_sums(a.row_sum + r0, a.dtype, T));
    a.utt_is_prob[u] = is_prob ? 1u : 0u;
    if (is_prob && a.utt_side) a.utt_side[u] = 3u;  // (time-sliced ingest: a slice was read as probabilities)
    if (is_prob) a.overflow[1] = 1u;  // flags[1]: some utterance needs the probability pass
  }
}

// per-wave LDS work area of the prune kernels
// leaves (<= 128 elements each) of numpy's pairwise sum a wave lists at a time: those of one 8192-element piece of a row
// (np_sum.h: at most NP_PIECE_LEAVES = 65), rounded up so that the work area stays a multiple of 16 bytes
constexpr int NP_LEAVES = 66;
static_assert(NP_LEAVES >= NP_PIECE_LEAVES, "a wave lists the leaves of a whole piece");
struct PruneLds {
  double* asc_lp;
  uint16_t *asc_id, *order, *tabA, *tabR, *scratch;
  double* np_sum;     // [NP_LEAVES + 16] leaf sums, then the combining stack (float64 rows: np_order_exp_sum)
  uint16_t* np_tab;   // [2 * NP_LEAVES + 48] leaf offsets, leaf lengths, two 16-entry stacks, the leaf count
};
constexpr size_t NP_LDS_BYTES = (NP_LEAVES + 16) * 8 + (((2 * NP_LEAVES + 48) * 2 + 15) & ~(size_t)15);
__host__ __device__ inline size_t prune_lds_bytes(size_t ms, size_t cap) {
  return (((ms + 1) * 8 + 15) & ~(size_t)15) + (((ms + 2) * 2 * 2 + 15) & ~(size_t)15) +
         ((cap * 2 * 3 + 15) & ~(size_t)15) + NP_LDS_BYTES;
}
__device__ __forceinline__ PruneLds prune_lds(char* smem, int wave, uint32_t ms, uint32_t cap) {
  char* base = smem + prune_lds_bytes(ms, cap) * wave;
  PruneLds w;
  w.asc_lp = (double*)base;
  w.asc_id = (uint16_t*)(base + (((size_t)(ms + 1) * 8 + 15) & ~(size_t)15));
  w.order = w.asc_id + (ms + 2);
  w.tabA = (uint16_t*)((char*)w.asc_id + (((size_t)(ms + 2) * 2 * 2 + 15) & ~(size_t)15));
  w.tabR = w.tabA + cap;
  w.scratch = w.tabR + cap;
  w.np_sum = (double*)(base + prune_lds_bytes(ms, cap) - NP_LDS_BYTES);
  w.np_tab = (uint16_t*)(w.np_sum + NP_LEAVES + 16);
  return w;
}

// numpy.argmax semantics on a row that may hold NaN (non-finite input rows): the first NaN wins, else the
// first maximum. (best, best_id) start as (-inf, INT_MAX); ids arrive in ascending order inside a lane.
__device__ __forceinline__ void argmax_take(double y, int id, double& best, int& best_id) {
  const bool bnan = best != best;
  if (!bnan && (y != y || y > best)) {
    best = y;
    best_id = id;
  }
}
__device__ __forceinline__ void argmax_merge(double ob, int oi, double& best, int& best_id) {
  const bool bnan = best != best, onan = ob != ob;
  const bool take = onan ? (!bnan || oi < best_id) : (!bnan && (ob > best || (ob == best && oi < best_id)));
  if (take) {
    best = ob;
    best_id = oi;
  }
}

// Common tail: argmax across the wave (first maximum, like numpy), CPython-set ordering on lane 0,
// coalesced write of the ordered (id, logp) list.
// ---- CPython set order with the table spread over the wave -------------------------------------------
// The same algorithm as set_order.h (Objects/setobject.c: set_add_entry / set_insert_clean /
// set_table_resize / set_merge) for tables of at most 64 slots: slot k lives in lane k, the free-slot map is
// a wave-uniform 64-bit mask, keys are wave-uniform -- so a probe sequence is a handful of SCALAR
// instructions on that mask (the linear 10-slot window is one shift + ctz) instead of a lane-0 walk over LDS.
// Up to 18 keys (+ argmax) never need more than 64 slots: 8 -> 32 at the 5th key, 128 only at the 19th.
constexpr uint32_t WAVE_SET_MAX_KEYS = 18;
struct WTab {
  uint32_t val;    // this lane's slot (SET_EMPTY when free)
  uint64_t empty;  // bit k: slot k is free            (uniform)
  uint32_t mask;   // table size - 1                   (uniform)
  uint32_t used;   //                                  (uniform)
};
__device__ __forceinline__ uint64_t wt_all(uint32_t size) { return size >= 64u ? ~0ull : ((1ull << size) - 1ull); }
__device__ __forceinline__ void wt_clear(WTab& t, uint32_t size) {
  t.val = SET_EMPTY;
  t.mask = size - 1u;
  t.used = 0;
  t.empty = wt_all(size);
}
__device__ __forceinline__ void wt_put(WTab& t, int lane, uint32_t pos, uint32_t key) {
  if ((uint32_t)lane == pos) t.val = key;
  t.empty &= ~(1ull << pos);
}
__device__ __forceinline__ void wt_insert_clean(WTab& t, int lane, uint32_t key) {  // set_insert_clean
  const uint32_t mask = t.mask;
  uint32_t perturb = key, i = key & mask;
  for (;;) {
    const uint64_t win = (t.empty >> i) & ((i + 9u <= mask) ? 0x3FFull : 1ull);  // slot i and the 9 after it
    if (win) {
      wt_put(t, lane, i + (uint32_t)__builtin_ctzll(win), key);
      return;
    }
    perturb >>= 5;
    i = (i * 5u + 1u + perturb) & mask;
  }
}
// every occupied slot of `src`, in slot order, re-inserted into `dst`
__device__ __forceinline__ void wt_reinsert(WTab& dst, int lane, uint32_t src_val, uint64_t src_occ) {
  while (src_occ) {
    const uint32_t k = (uint32_t)__builtin_ctzll(src_occ);
    src_occ &= src_occ - 1ull;
    const uint32_t key = (uint32_t)__builtin_amdgcn_readlane((int)src_val, (int)k);
    wt_insert_clean(dst, lane, key);
  }
}
__device__ __forceinline__ void wt_resize(WTab& t, int lane, uint32_t minused) {  // set_table_resize
  uint32_t newsize = 8;
  while (newsize <= minused) newsize <<= 1;
  const uint32_t old_val = t.val, used = t.used;
  const uint64_t occ = ~t.empty & wt_all(t.mask + 1u);
  wt_clear(t, newsize);
  t.used = used;
  wt_reinsert(t, lane, old_val, occ);
}
__device__ __forceinline__ void wt_add(WTab& t, int lane, uint32_t key) {  // set_add_entry
  const uint32_t mask = t.mask;
  const uint64_t same = __ballot(t.val == key);
  uint32_t perturb = key, i = key & mask;
  for (;;) {
    const uint64_t winmask = (i + 9u <= mask) ? 0x3FFull : 1ull;
    const uint64_t we = (t.empty >> i) & winmask, ws = (same >> i) & winmask;
    if (we | ws) {
      const uint32_t first = (uint32_t)__builtin_ctzll(we | ws);
      if ((ws >> first) & 1ull) return;  // already a member
      wt_put(t, lane, i + first, key);
      t.used += 1u;
      if (t.used * 5u >= mask * 3u) wt_resize(t, lane, t.used > 50000u ? t.used * 2u : t.used * 4u);
      return;
    }
    perturb >>= 5;
    i = (i * 5u + 1u + perturb) & mask;
  }
}
// set(asc[0..n)) | {argmax} for n <= WAVE_SET_MAX_KEYS: returns the member count; this lane's slot value and
// the occupancy mask (slot order = iteration order) come back through the references.
__device__ __forceinline__ uint32_t wave_set_order(const uint16_t* asc, uint32_t n, uint32_t argmax, int lane,
                                                   uint32_t& my_val, uint64_t& occ) {
  WTab a, r;
  wt_clear(a, 8);
  for (uint32_t k = 0; k < n; ++k) wt_add(a, lane, (uint32_t)__builtin_amdgcn_readfirstlane((int)asc[k]));
  wt_clear(r, 8);
  if (a.used) {  // set_merge (the `|` copies the left operand first)
    if (a.used * 5u >= r.mask * 3u) {
      uint32_t newsize = 8;
      while (newsize <= a.used * 2u) newsize <<= 1;
      wt_clear(r, newsize);
    }
    if (r.mask == a.mask) {
      r.val = a.val;
      r.empty = a.empty;
    } else {
      wt_reinsert(r, lane, a.val, ~a.empty & wt_all(a.mask + 1u));
    }
    r.used = a.used;
  }
  if ((r.used + 1u) * 5u >= r.mask * 3u) wt_resize(r, lane, (r.used + 1u) * 2u);
  wt_add(r, lane, argmax);
  my_val = r.val;
  occ = ~r.empty & wt_all(r.mask + 1u);
  return (uint32_t)__popcll(occ);
}

__device__ __forceinline__ void prune_finish(const PruneArgs& a, int64_t row, int lane, const PruneLds& w, uint32_t n,
                                             double best, int best_id, bool reduced = false) {
  const uint32_t ms = (uint32_t)a.max_surv;
  bool overflow = false;
  if (n > ms) {
    overflow = true;
    n = ms;
  }
  if (!reduced) {  // (best, best_id) are per-lane candidates: reduce across the wave
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      double ob = __shfl_xor(best, off, 64);
      int oi = __shfl_xor(best_id, off, 64);
      argmax_merge(ob, oi, best, best_id);
    }
  }
  __builtin_amdgcn_wave_barrier();
  __threadfence_block();
  uint16_t* out_id = a.surv_id + (size_t)row * ms;
  double* out_lp = a.surv_lp + (size_t)row * ms;
  if (n <= WAVE_SET_MAX_KEYS) {  // the usual frame: a handful of survivors, table in registers
    uint32_t my_id = SET_EMPTY;
    uint64_t occ = 0;
    uint32_t m = wave_set_order(w.asc_id, n, (uint32_t)__builtin_amdgcn_readfirstlane(best_id), lane, my_id, occ);
    const uint32_t pos = (uint32_t)__popcll(occ & ((1ull << lane) - 1ull));
    if (m > ms) {
      overflow = true;
      m = ms;
    }
    if (lane == 0) {
      a.surv_cnt[row] = m;
      if (overflow) a.overflow[0] = 1u;
    }
    if (((occ >> lane) & 1ull) && pos < m) {
      double lp = best;  // the argmax may be absent from the list (below the threshold)
      for (uint32_t k = 0; k < n; ++k)
        if (w.asc_id[k] == my_id) lp = w.asc_lp[k];
      out_id[pos] = (uint16_t)my_id;
      out_lp[pos] = lp;
    }
    return;
  }
  uint32_t m = 0;
  if (lane == 0) m = cpython_set_order(w.asc_id, n, (uint32_t)best_id, w.tabA, w.tabR, w.scratch, w.order);
  m = __shfl(m, 0, 64);
  __threadfence_block();
  if (m > ms) {
    overflow = true;
    m = ms;
  }
  if (lane == 0) {
    a.surv_cnt[row] = m;
    if (overflow) a.overflow[0] = 1u;
  }
  for (uint32_t k = lane; k < m; k += 64) {
    uint32_t id = w.order[k];
    // binary search the ascending list for the log-prob (the argmax may be absent: below threshold)
    double lp = best;
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
      uint32_t mid = (lo + hi) >> 1;
      if (w.asc_id[mid] < id) lo = mid + 1; else hi = mid;
    }
    if (lo < n && w.asc_id[lo] == id) lp = w.asc_lp[lo];
    out_id[k] = (uint16_t)id;
    out_lp[k] = lp;
  }
}

__device__ __forceinline__ double to_logp(double xv, bool is_prob, double mx, double lse) {
  const double clip_lo = -34.538776394910684;  // ln(1e-15)
  if (is_prob) {
    double p = xv < 1e-15 ? 1e-15 : (xv > 1.0 ? 1.0 : xv);
    return log(p);
  }
  double y = (xv - mx) - lse;
  return y < clip_lo ? clip_lo : (y > 0.0 ? 0.0 : y);
}

// float32 rows in the reference's own arithmetic (decoder.py:180-197 and :762 on a float32 array): (x - max) - log(sum) in
// float32 with numpy's float32 log (np_f32.h), widened by the clip; probability rows: numpy's float32 log of the float32 clip.
__device__ __forceinline__ double to_logp_np32(float xv, bool is_prob, float mf, float l32) {
  const double clip_lo = -34.538776394910684;  // ln(1e-15)
  if (is_prob) {
    const float lo = (float)1e-15;
    const float p = xv < lo ? lo : (xv > 1.0f ? 1.0f : xv);  // (NaN stays NaN, like np.clip)
    return (double)np_log_f32(p);
  }
  const float t = xv - mf;
  const double y = (double)(t - l32);
  return y < clip_lo ? clip_lo : (y > 0.0 ? 0.0 : y);
}

// float64 rows: sum_v exp(x[v] - m) in the order numpy's np.sum adds a contiguous float64 row (pairwise: np_sum.h), by one
// wave. The reference's log-softmax (decoder.py:180-197) is x - max - log(np.sum(np.exp(x - max))): with the normaliser
// summed in this order a frame's log-probabilities are the reference's own bit for bit wherever exp / log round like
// numpy's, and with them the order inside runs of equal scores (tests/test_order_stability.py). Leaves of the recursion
// (<= 128 elements: eight strided accumulators, then the leftovers) go to groups of eight lanes, eight leaves at a time;
// lane 0 lists them first and combines their sums last, both by walking the recursion with a small stack in LDS.
// numpy runs that recursion on pieces of NP_PIECE = 8192 elements and adds the pieces' sums to the result one after the other
// (np_sum.h), so does the loop here: a piece has at most NP_PIECE_LEAVES <= NP_LEAVES leaves and a recursion depth of 7, which
// is all the work area has to hold for any row up to CTCDEC_MAX_VOCAB = 65535 labels.
// T = double: the terms are exp(x - m) in fp64; T = float: numpy's float32 exp of the float32 difference, float32 additions
// (the leaf sums travel through the fp64 LDS words unchanged: every float32 is a double).
template <typename T>
__device__ __forceinline__ T np_term(const T* x, int i, T m);
template <>
__device__ __forceinline__ double np_term<double>(const double* x, int i, double m) { return exp(x[i] - m); }
template <>
__device__ __forceinline__ float np_term<float>(const float* x, int i, float m) { return np_exp_f32(x[i] - m); }
// one piece: elements [p0, p0 + pn) of the row, pn <= NP_PIECE (p0 + pn <= 65535: label ids, and so the offsets, are 16 bits wide)
template <typename T>
__device__ __forceinline__ T np_order_exp_sum_piece(const T* x, int p0, int pn, T m, int lane, const PruneLds& w) {
  uint16_t* leaf_off = w.np_tab;
  uint16_t* leaf_len = w.np_tab + NP_LEAVES;
  uint16_t* stk_n = w.np_tab + 2 * NP_LEAVES;
  uint16_t* stk_s = stk_n + 16;
  uint16_t* n_leaf = stk_s + 16;
  if (lane == 0) {  // the piece's leaves, left to right
    int sp = 0, k = 0;
    stk_s[0] = (uint16_t)p0;
    stk_n[0] = (uint16_t)pn;
    sp = 1;
    while (sp > 0) {
      --sp;
      const int off = stk_s[sp], n = stk_n[sp];
      if (n <= 128) {
        if (k < NP_LEAVES) {  // (always: a piece has at most NP_PIECE_LEAVES of them)
          leaf_off[k] = (uint16_t)off;
          leaf_len[k] = (uint16_t)n;
          ++k;
        }
      } else if (sp + 2 <= 16) {  // (always: the halves of 8192 reach 128 at depth 6, one pending right half per level)
        int n2 = n / 2;
        n2 -= n2 % 8;
        stk_s[sp] = (uint16_t)(off + n2);  // right half below the left one: the left is listed first
        stk_n[sp] = (uint16_t)(n - n2);
        stk_s[sp + 1] = (uint16_t)off;
        stk_n[sp + 1] = (uint16_t)n2;
        sp += 2;
      }
    }
    *n_leaf = (uint16_t)k;
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const int nl = *n_leaf;
  const int g = lane >> 3, j = lane & 7;
  for (int base = 0; base < nl; base += 8) {
    const int k = base + g;
    const bool mine = k < nl;
    const int off = mine ? leaf_off[k] : 0, n = mine ? leaf_len[k] : 0;
    T res = (T)0;
    if (n < 8) {
      for (int i = 0; i < n; ++i) res = res + np_term<T>(x, off + i, m);
    } else {
      T r = np_term<T>(x, off + j, m);
      const int body = n - (n % 8);
      for (int i = 8; i < body; i += 8) r = r + np_term<T>(x, off + i + j, m);
      // ((r0+r1)+(r2+r3)) + ((r4+r5)+(r6+r7)): additions commute, so an xor butterfly inside the group is that very tree
      r = r + __shfl_xor(r, 1, 64);
      r = r + __shfl_xor(r, 2, 64);
      r = r + __shfl_xor(r, 4, 64);
      res = r;
      for (int i = body; i < n; ++i) res = res + np_term<T>(x, off + i, m);
    }
    if (mine && j == 0) w.np_sum[k] = (double)res;
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
  if (lane == 0) {  // pairwise(a, n2) + pairwise(a + n2, n - n2), all the way up
    double* acc = w.np_sum + NP_LEAVES;
    uint16_t* stk_st = stk_s;
    int sp = 1, k = 0;
    stk_n[0] = (uint16_t)pn;
    stk_st[0] = 0;
    T ret = (T)0;
    while (sp > 0) {
      const int n = stk_n[sp - 1], st = stk_st[sp - 1];
      if (n <= 128) {
        ret = (T)w.np_sum[k++];
        --sp;
        continue;
      }
      int n2 = n / 2;
      n2 -= n2 % 8;
      if (st == 0) {
        stk_st[sp - 1] = 1;
        stk_n[sp] = (uint16_t)n2;
        stk_st[sp] = 0;
        ++sp;
      } else if (st == 1) {
        acc[sp - 1] = (double)ret;
        stk_st[sp - 1] = 2;
        stk_n[sp] = (uint16_t)(n - n2);
        stk_st[sp] = 0;
        ++sp;
      } else {
        ret = (T)acc[sp - 1] + ret;
        --sp;
      }
    }
    w.np_sum[0] = (double)ret;
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const T sum = (T)w.np_sum[0];
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();  // (the next piece, or the caller, writes the work area again)
  return sum;
}
template <typename T>
__device__ __forceinline__ T np_order_exp_sum(const T* x, int V, T m, int lane, const PruneLds& w) {
  T out = (T)0;  // (numpy's output element starts at 0, and 0 + s is s: a sum of exponentials is never -0)
  for (int p0 = 0; p0 < V; p0 += (int)NP_PIECE)
    out = out + np_order_exp_sum_piece<T>(x, p0, V - p0 < (int)NP_PIECE ? V - p0 : (int)NP_PIECE, m, lane, w);
  return out;
}

// Generic frame-prune: one wave per frame row, any V / dtype; the row is swept three times (max and
// row sum, sum of exponentials, selection) and stays in L1/L2 between sweeps.
// pass 0: every utterance is treated as logits (the overwhelmingly common case) and the row sums for the
//         probability sniff are produced on the way; pass 1 (only launched when utt_sniff found
//         probability-like utterances) redoes just those utterances with log(clip(p)).
template <typename T>
__device__ __forceinline__ void prune_row_generic(const PruneArgs& a, int64_t row, const PruneLds& w, int lane) {
  const int V = a.n_labels;
  const int u = find_utt(a.utt_row0, a.n_utts, row);
  const bool is_prob = a.pass == 1;
  if (is_prob && a.utt_is_prob[u] != 1u) return;
  const T* x = (const T*)a.utt_logits[u] + (size_t)(row - a.utt_row0[u]) * V;
  double mx = 0.0, lse = 0.0;
  // float32 rows: the reference's own float32 arithmetic (to_logp_np32) unless CTCDEC_PRUNE_EXP asks for fp64
  constexpr bool F32 = std::is_same<T, float>::value;
  const bool np32 = F32 && a.f32_np;
  float mf = 0.f, l32 = 0.f;
  if (!is_prob) {
    double m = -INFINITY, rs = 0.0;
    for (int v = lane; v < V; v += 64) {
      double xv = ld(x, v);
      m = fmax(m, xv);
      rs += xv;
    }
    m = wave_max(m);
    rs = wave_sum(rs);
    if (lane == 0) a.row_sum[row] = rs;
    if (!isfinite(m)) m = 0.0;  // decoder.py:186-189
    if constexpr (F32) {
      if (np32) {
        mf = (float)m;  // (exact: the maximum of float32 values)
        l32 = np_log_f32(np_order_exp_sum<float>((const float*)x, V, mf, lane, w));
      }
    }
    if (!np32) {
      double s = 0.0;
      if constexpr (std::is_same<T, double>::value) {  // float64 rows: numpy's own summation order
        s = np_order_exp_sum<double>(x, V, m, lane, w);
      } else {  // 16-bit rows, float32 rows in fp64 mode: the log-softmax of the exact upcast, summed in lane order
        for (int v = lane; v < V; v += 64) s += exp(ld(x, v) - m);
        s = wave_sum(s);
      }
      lse = log(s);
    }
    mx = m;
  }
  uint32_t n = 0;
  double best = -INFINITY;
  int best_id = 0x7FFFFFFF;
  const uint32_t ms = (uint32_t)a.max_surv;
  for (int v0 = 0; v0 < V; v0 += 64) {
    int v = v0 + lane;
    double y = -INFINITY;
    bool in = v < V;
    if (in) {
      if constexpr (F32) y = np32 ? to_logp_np32(((const float*)x)[v], is_prob, mf, l32) : to_logp(ld(x, v), is_prob, mx, lse);
      else y = to_logp(ld(x, v), is_prob, mx, lse);
      argmax_take(y, v, best, best_id);
    }
    bool keep = in && y >= a.token_min_logp;
    unsigned long long mask = __ballot(keep);
    if (keep) {
      uint32_t pos = n + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
      if (pos < ms) {
        w.asc_id[pos] = (uint16_t)v;
        w.asc_lp[pos] = y;
      }
    }
    n += (uint32_t)__popcll(mask);
  }
  prune_finish(a, row, lane, w, n, best, best_id);
}
template <typename T>
__global__ __launch_bounds__(PRUNE_WAVES * 64) void frame_prune(PruneArgs a, uint32_t cap) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t row = a.row_base + (int64_t)blockIdx.x * PRUNE_WAVES + wave;
  if (row >= a.row_base + a.n_rows) return;
  prune_row_generic<T>(a, row, prune_lds(smem, wave, (uint32_t)a.max_surv, cap), lane);
}
// the rows frame_prune_fast left on its list for 16-bit inputs (a.slow_rows, a.overflow[3] of them), one wave per row
template <typename T>
__global__ __launch_bounds__(PRUNE_WAVES * 64) void frame_prune_listed(PruneArgs a, uint32_t cap) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const PruneLds w = prune_lds(smem, wave, (uint32_t)a.max_surv, cap);
  const uint32_t count = a.overflow[3];
  for (uint32_t k = blockIdx.x * PRUNE_WAVES + wave; k < count; k += gridDim.x * PRUNE_WAVES) {
    prune_row_generic<T>(a, a.row_base + (int64_t)a.slow_rows[k], w, lane);
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();
  }
}

// exp(d) for d <= 0 (d = logit - row max), fp64, ~1 ulp: 2^k * exp(r) with k = rint(d / ln 2), |r| <= ln2/2,
// exp(r) by its degree-13 Taylor polynomial (next term < 5e-18 relative). No overflow side to handle and the
// underflow side is a clamp, which is what makes it ~2/3 of the general routine's instructions.
__device__ __forceinline__ double exp_nonpos(double d) {
  d = fmax(d, -750.0);  // exp(-750) == 0 in fp64; also maps -inf (masked labels) to 0
  const double kf = rint(d * 1.44269504088896338700e+00);
  double r = fma(kf, -6.93147180369123816490e-01, d);
  r = fma(kf, -1.90821492927058770002e-10, r);
  double p = 1.6059043836821613e-10;            // 1/13!
  p = fma(p, r, 2.08767569878680990e-09);       // 1/12!
  p = fma(p, r, 2.50521083854417188e-08);       // 1/11!
  p = fma(p, r, 2.75573192239858907e-07);       // 1/10!
  p = fma(p, r, 2.75573192239858907e-06);       // 1/9!
  p = fma(p, r, 2.48015873015873016e-05);       // 1/8!
  p = fma(p, r, 1.98412698412698413e-04);       // 1/7!
  p = fma(p, r, 1.38888888888888889e-03);       // 1/6!
  p = fma(p, r, 8.33333333333333333e-03);       // 1/5!
  p = fma(p, r, 4.16666666666666667e-02);       // 1/4!
  p = fma(p, r, 1.66666666666666667e-01);       // 1/3!
  p = fma(p, r, 5.00000000000000000e-01);
  p = fma(p, r, 1.0);
  p = fma(p, r, 1.0);
  return ldexp(p, (int)kf);
}

// The same with the degree-9 polynomial: relative error < 7e-12 (|r|^10 / 10!), for sums that feed a float32 input's
// log-softmax (frame_prune_f32x4); four FMAs less per call.
__device__ __forceinline__ double exp_nonpos9(double d) {
  d = fmax(d, -750.0);
  const double kf = rint(d * 1.44269504088896338700e+00);
  double r = fma(kf, -6.93147180369123816490e-01, d);
  r = fma(kf, -1.90821492927058770002e-10, r);
  double p = 2.75573192239858907e-06;           // 1/9!
  p = fma(p, r, 2.48015873015873016e-05);       // 1/8!
  p = fma(p, r, 1.98412698412698413e-04);       // 1/7!
  p = fma(p, r, 1.38888888888888889e-03);       // 1/6!
  p = fma(p, r, 8.33333333333333333e-03);       // 1/5!
  p = fma(p, r, 4.16666666666666667e-02);       // 1/4!
  p = fma(p, r, 1.66666666666666667e-01);       // 1/3!
  p = fma(p, r, 5.00000000000000000e-01);
  p = fma(p, r, 1.0);
  p = fma(p, r, 1.0);
  return ldexp(p, (int)kf);
}

// float32 exp(d), d <= 0, two at a time (v_pk_* math): degree-8 Taylor polynomial after a two-constant argument reduction,
// every step one rounding (fma). Measured on the host with the same operations (tools/exp_f32_study.c, 20 M arguments in
// [-14, 0]): mean relative error 1.5e-11 (libm's expf: 3.5e-11), mean |error| 2.2e-8, maximum 7.4e-8 -- i.e. what numpy's
// float32 exp gives the reference (decoder.py:180-197), and without the one-sided error of v_exp_f32. Arguments below -80
// (incl. -inf masks) are clamped: exp(-80) = 1.8e-35 does not register in a sum >= 1.
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 exp_nonpos_f32x2(f32x2 d) {
  d = __builtin_elementwise_max(d, (f32x2)(-80.0f));
  const f32x2 n = __builtin_elementwise_roundeven(d * (f32x2)(1.44269504088896340736f));
  f32x2 r = __builtin_elementwise_fma(n, (f32x2)(-0.693145751953125f), d);
  r = __builtin_elementwise_fma(n, (f32x2)(-1.42860682030941723212e-6f), r);
  f32x2 p = (f32x2)(2.48015873015873016e-05f);                              // 1/8!
  p = __builtin_elementwise_fma(p, r, (f32x2)(1.98412698412698413e-04f));   // 1/7!
  p = __builtin_elementwise_fma(p, r, (f32x2)(1.38888888888888889e-03f));   // 1/6!
  p = __builtin_elementwise_fma(p, r, (f32x2)(8.33333333333333333e-03f));   // 1/5!
  p = __builtin_elementwise_fma(p, r, (f32x2)(4.16666666666666667e-02f));   // 1/4!
  p = __builtin_elementwise_fma(p, r, (f32x2)(1.66666666666666667e-01f));   // 1/3!
  p = __builtin_elementwise_fma(p, r, (f32x2)(0.5f));
  p = __builtin_elementwise_fma(p, r, (f32x2)(1.0f));
  p = __builtin_elementwise_fma(p, r, (f32x2)(1.0f));
  f32x2 out;
  out.x = ldexpf(p.x, (int)n.x);
  out.y = ldexpf(p.y, (int)n.y);
  return out;
}

// log(s) for 1 <= s < 2^24, fp64: one Newton step on the fp32 logarithm -- y0 = logf(s), r = s * exp(-y0) - 1
// (|r| ~ 1e-6), log(s) = y0 + log1p(r) = y0 + r - r^2/2 (next term < 1e-18). A third of ocml's double-double log.
__device__ __forceinline__ double log_ge1(double s) {
  const double y0 = (double)__logf((float)s);
  const double r = fma(s, exp_nonpos(-y0), -1.0);
  return y0 + (r - 0.5 * r * r);
}

// Register-resident frame-prune for fp32 rows with V % 4 == 0 and V <= 1024*... (NC chunks of 256
// labels): each lane pulls its 4*NC logits with 16-byte loads ONCE (1 KiB per wave-instruction, fully
// coalesced) and all three sweeps run out of registers: the logits cross HBM exactly once.
// PK: the exponentials of the clean-row path as packed float32 polynomials (the default; CTCDEC_PRUNE_EXP=f64: fp64)
template <int NC, bool PK>
__device__ __forceinline__ void prune_row_f32x4(const PruneArgs& a, int64_t row, const PruneLds& w, int lane) {
  const int V = a.n_labels;
  const int u = find_utt(a.utt_row0, a.n_utts, row);
  const bool is_prob = a.pass == 1;
  if (is_prob && a.utt_is_prob[u] != 1u) return;
  const float4* x4 = (const float4*)((const float*)a.utt_logits[u] + (size_t)(row - a.utt_row0[u]) * V);
  const int n4 = V >> 2;
  float4 r[NC];
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    const int i4 = k * 64 + lane;
    r[k] = i4 < n4 ? x4[i4] : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
  }
  double mx = 0.0, lse = 0.0;
  const uint32_t ms = (uint32_t)a.max_surv;
  const unsigned long long lt = (1ull << lane) - 1ull;
  if (!is_prob) {
    float mf = -INFINITY;
    // The row sum only feeds utt_sniff's coarse "could these be probabilities?" test (|mean row sum - 1| <= 0.5; the exact
    // test in numpy's own order is utt_sniff_exact's): each lane adds its <= 16 values in float32 (error < 2e-5 for
    // logits up to +-20, nothing for probabilities), the wave sum is fp64.
    float rsf = 0.f;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      if (k * 64 + lane < n4) {
        mf = fmaxf(fmaxf(mf, fmaxf(r[k].x, r[k].y)), fmaxf(r[k].z, r[k].w));
        rsf += (r[k].x + r[k].y) + (r[k].z + r[k].w);
      }
    }
    double m = wave_max((double)mf);
    double rs = wave_sum((double)rsf);
    if (lane == 0) a.row_sum[row] = rs;
    // ---- the clean row (finite maximum, no NaN: -inf masks are fine): everything below in its cheapest form
    if (isfinite(m) && rs == rs) {
      // The reference computes the log-softmax of float32 logits IN float32 (decoder.py:180-197: np.exp / np.sum on
      // the float32 array, correctly rounded per term, errors of either sign). Tried and dropped: v_exp_f32 -- a
      // third of the instructions, but the hardware exp2 errs to one side, which shifts lse by ~5e-8 in EVERY frame and
      // the scores by 4.8e-5 over T=1000 (tools/golden_full_gap.py; the bound is 1e-4). Kept: the fp64 routine cut to
      // the degree its purpose needs (1e-11 per term, errors of either sign), fp64 accumulation.
      const float mfw = (float)m;  // exact: m is the maximum of float32 values
      double sl = 0.0;
      // round 6: the reference's float32 arithmetic itself (numpy's float32 exp, its pairwise float32 sum, its float32 log:
      // np_f32.h, np_order_exp_sum<float>; the row is read a second time, from L1 / L2) -- a frame's log-probabilities are the
      // reference's bits. The polynomial variants below stay for CTCDEC_PRUNE_EXP=pk / f64.
      float l32 = 0.f;
      const bool np32 = a.f32_np != 0;
      if (np32) l32 = np_log_f32(np_order_exp_sum<float>((const float*)x4, V, mfw, lane, w));
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        if (!np32 && k * 64 + lane < n4) {
          if (PK) {
            // (x - m in float32: one rounding, as in the reference's float32 `x - x_max`)
            const f32x2 e01 = exp_nonpos_f32x2((f32x2){r[k].x - mfw, r[k].y - mfw});
            const f32x2 e23 = exp_nonpos_f32x2((f32x2){r[k].z - mfw, r[k].w - mfw});
            sl += ((double)e01.x + (double)e01.y) + ((double)e23.x + (double)e23.y);
          } else {
            sl += (exp_nonpos9((double)r[k].x - m) + exp_nonpos9((double)r[k].y - m)) +
                  (exp_nonpos9((double)r[k].z - m) + exp_nonpos9((double)r[k].w - m));
          }
        }
      }
      if (!np32) {
        const double s = wave_sum(sl);
        lse = log_ge1(s);
      } else {
        lse = (double)l32;
      }
      // argmax of the log-probs = first maximum of the logits (x -> clip(x - m - lse) is monotone, and two
      // different fp32 logits never round to the same fp64 value after the two subtractions)
      int first = 0x7FFFFFFF;
#pragma unroll
      for (int k = NC - 1; k >= 0; --k) {
        const int v0 = (k * 64 + lane) * 4;
        if (k * 64 + lane < n4) {
          first = r[k].w == mfw ? v0 + 3 : first;
          first = r[k].z == mfw ? v0 + 2 : first;
          first = r[k].y == mfw ? v0 + 1 : first;
          first = r[k].x == mfw ? v0 : first;
        }
      }
      first = wave_min_i32(first);
      const double best = np32 ? to_logp_np32(mfw, false, mfw, l32) : to_logp((double)mfw, false, m, lse);
      // survivors: an fp32 screen that cannot miss (threshold rounded down, with a margin far above the fp64
      // rounding of the exact test), then the exact fp64 test only in the 256-label chunks that have a candidate
      const double xthr = m + lse + a.token_min_logp;
      // (a threshold at or below the clip keeps every label: decoder.py:444 tests the clipped values)
      // (float32 arithmetic: two roundings of up to half an ulp of |x - m| and |y| each -- a wider margin)
      const float pre = a.token_min_logp <= -34.538776394910684 ? -INFINITY
                                                                  : __double2float_rd(xthr - (np32 ? 3e-5 * (4.0 + fabs(xthr)) : 1e-6 * (1.0 + fabs(xthr))));
      uint32_t n = 0;
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        const bool in = k * 64 + lane < n4;
        const bool cand = in && (r[k].x >= pre || r[k].y >= pre || r[k].z >= pre || r[k].w >= pre);
        if (__ballot(cand)) {
          const int v0 = (k * 64 + lane) * 4;
          double y0 = -INFINITY, y1 = -INFINITY, y2 = -INFINITY, y3 = -INFINITY;
          if (cand && np32) {
            y0 = to_logp_np32(r[k].x, false, mfw, l32);
            y1 = to_logp_np32(r[k].y, false, mfw, l32);
            y2 = to_logp_np32(r[k].z, false, mfw, l32);
            y3 = to_logp_np32(r[k].w, false, mfw, l32);
          } else if (cand) {
            y0 = to_logp((double)r[k].x, false, m, lse);
            y1 = to_logp((double)r[k].y, false, m, lse);
            y2 = to_logp((double)r[k].z, false, m, lse);
            y3 = to_logp((double)r[k].w, false, m, lse);
          }
          const bool k0 = cand && y0 >= a.token_min_logp, k1 = cand && y1 >= a.token_min_logp;
          const bool k2 = cand && y2 >= a.token_min_logp, k3 = cand && y3 >= a.token_min_logp;
          const unsigned long long b0 = __ballot(k0), b1 = __ballot(k1), b2 = __ballot(k2), b3 = __ballot(k3);
          uint32_t pos = n + (uint32_t)(__popcll(b0 & lt) + __popcll(b1 & lt) + __popcll(b2 & lt) + __popcll(b3 & lt));
          if (k0) { if (pos < ms) { w.asc_id[pos] = (uint16_t)v0; w.asc_lp[pos] = y0; } ++pos; }
          if (k1) { if (pos < ms) { w.asc_id[pos] = (uint16_t)(v0 + 1); w.asc_lp[pos] = y1; } ++pos; }
          if (k2) { if (pos < ms) { w.asc_id[pos] = (uint16_t)(v0 + 2); w.asc_lp[pos] = y2; } ++pos; }
          if (k3) { if (pos < ms) { w.asc_id[pos] = (uint16_t)(v0 + 3); w.asc_lp[pos] = y3; } ++pos; }
          n += (uint32_t)(__popcll(b0) + __popcll(b1) + __popcll(b2) + __popcll(b3));
        }
      }
      prune_finish(a, row, lane, w, n, best, first, /*reduced=*/true);
      return;
    }
    if (!isfinite(m)) m = 0.0;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
      if (k * 64 + lane < n4)
        s += (exp((double)r[k].x - m) + exp((double)r[k].y - m)) + (exp((double)r[k].z - m) + exp((double)r[k].w - m));
    }
    s = wave_sum(s);
    mx = m;
    lse = log(s);
  }
  uint32_t n = 0;
  double best = -INFINITY;
  int best_id = 0x7FFFFFFF;
#pragma unroll
  for (int k = 0; k < NC; ++k) {
    const bool in = k * 64 + lane < n4;
    const int v0 = (k * 64 + lane) * 4;
    double y0 = -INFINITY, y1 = -INFINITY, y2 = -INFINITY, y3 = -INFINITY;
    if (in && is_prob && a.f32_np) {  // (probability rows: numpy's float32 log of the float32 clip)
      y0 = to_logp_np32(r[k].x, true, 0.f, 0.f);
      y1 = to_logp_np32(r[k].y, true, 0.f, 0.f);
      y2 = to_logp_np32(r[k].z, true, 0.f, 0.f);
      y3 = to_logp_np32(r[k].w, true, 0.f, 0.f);
    } else if (in) {
      y0 = to_logp((double)r[k].x, is_prob, mx, lse);
      y1 = to_logp((double)r[k].y, is_prob, mx, lse);
      y2 = to_logp((double)r[k].z, is_prob, mx, lse);
      y3 = to_logp((double)r[k].w, is_prob, mx, lse);
    }
    if (in) {
      argmax_take(y0, v0, best, best_id);
      argmax_take(y1, v0 + 1, best, best_id);
      argmax_take(y2, v0 + 2, best, best_id);
      argmax_take(y3, v0 + 3, best, best_id);
    }
    const bool k0 = in && y0 >= a.token_min_logp, k1 = in && y1 >= a.token_min_logp;
    const bool k2 = in && y2 >= a.token_min_logp, k3 = in && y3 >= a.token_min_logp;
    const unsigned long long any = __ballot(k0 || k1 || k2 || k3);
    if (any) {  // ascending id order inside the chunk = (lane, element)
      const unsigned long long b0 = __ballot(k0), b1 = __ballot(k1), b2 = __ballot(k2), b3 = __ballot(k3);
      uint32_t pos = n + (uint32_t)(__popcll(b0 & lt) + __popcll(b1 & lt) + __popcll(b2 & lt) + __popcll(b3 & lt));
      if (k0) { if (pos < ms) { w.asc_id[pos] = (uint16_t)v0; w.asc_lp[pos] = y0; } ++pos; }
      if (k1) { if (pos < ms) { w.asc_id[pos] = (uint16_t)(v0 + 1); w.asc_lp[pos] = y1; } ++pos; }
      if (k2) { if (pos < ms) { w.asc_id[pos] = (uint16_t)(v0 + 2); w.asc_lp[pos] = y2; } ++pos; }
      if (k3) { if (pos < ms) { w.asc_id[pos] = (uint16_t)(v0 + 3); w.asc_lp[pos] = y3; } ++pos; }
      n += (uint32_t)(__popcll(b0) + __popcll(b1) + __popcll(b2) + __popcll(b3));
    }
  }
  prune_finish(a, row, lane, w, n, best, best_id);
}
template <int NC, bool PK>
__global__ __launch_bounds__(PRUNE_WAVES * 64) void frame_prune_f32x4(PruneArgs a, uint32_t cap) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t row = a.row_base + (int64_t)blockIdx.x * PRUNE_WAVES + wave;
  if (row >= a.row_base + a.n_rows) return;
  prune_row_f32x4<NC, PK>(a, row, prune_lds(smem, wave, (uint32_t)a.max_surv, cap), lane);
}
// the rows frame_prune_fast left on its list (a.slow_rows, a.overflow[3] of them), one wave per row
template <int NC>
__global__ __launch_bounds__(PRUNE_WAVES * 64) void frame_prune_f32x4_listed(PruneArgs a, uint32_t cap) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const PruneLds w = prune_lds(smem, wave, (uint32_t)a.max_surv, cap);
  const uint32_t count = a.overflow[3];
  for (uint32_t k = blockIdx.x * PRUNE_WAVES + wave; k < count; k += gridDim.x * PRUNE_WAVES) {
    prune_row_f32x4<NC, true>(a, a.row_base + (int64_t)a.slow_rows[k], w, lane);
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();
  }
}

// ---------------------------------------------------------------------------------------------
// frame_prune_fast: 64 frames per wavefront, in two phases
// ---------------------------------------------------------------------------------------------
// The per-row kernel above spends most of its instructions on what follows the log-softmax: finding the survivors, ordering
// them the way a CPython set would, writing them out -- a serial tail of a few hundred instructions that 63 of the 64 lanes
// sit through. Here a wave takes 64 consecutive rows and
//   phase A (one row at a time, 64 lanes x 16 logits, the next row's loads in flight): row maximum and sum, the sum of
//     exponentials (packed float32 polynomials, see exp_nonpos_f32x2m), the first maximum, and the labels that pass a float32
//     screen of the threshold, left UNORDERED in a 16-slot LDS column of the row; the row's scalars land in lane `row`;
//   phase B (one row per LANE): the exact fp64 test of the candidates, an insertion sort by label id, the CPython set order
//     (set_order_small.h: 48 table slots per lane) and the output records -- the serial tail, 64 rows at a time.
// Rows this does not cover (non-finite maximum or NaN, more than 16 candidates / 15 survivors, survivor counts at the
// max_surv bound) go onto a list and frame_prune_f32x4_listed runs the per-row code on them right behind this kernel.
constexpr int PF_ROWS = 64;   // rows per wave (phase B: one per lane)
constexpr int PF_CAND = 16;   // candidates a row may leave for phase B
constexpr int PF_WAVES = 3;   // waves per SIMD the kernel is compiled for up to 1024 labels (NC <= 4)
constexpr int NP_IL = 2;      // groups of four labels whose exponentials are interleaved stage by stage (NP)
constexpr size_t PF_LDS_IDS = (size_t)PF_ROWS * PF_CAND * 2;
constexpr size_t PF_LDS_X = (size_t)PF_ROWS * PF_CAND * 4;
static_assert(PRUNE_FAST_MAX_LABELS - 1 <= (int)SMALL_SET_MAX_ID, "label ids must fit the small set tables");
constexpr size_t PF_LDS = PF_LDS_IDS + PF_LDS_X + (size_t)PF_ROWS * SMALL_SET_SLOTS * 2;  // 12 KiB: 13 waves per CU

// exp(d), d <= 0, two at a time, as exp_nonpos_f32x2 with the rounding and the scaling done by the 1.5 * 2^23 trick
// (t = d * log2(e) + magic holds round(d * log2 e) in its low mantissa bits: n = t - magic, and bits(t) << 23 is n in the
// exponent field: 2^n * p is one integer add, no v_rndne / v_cvt / v_ldexp) and the degree-7 polynomial. Same operations
// on the host (20 M arguments in [-14, 0]): mean relative error -5.8e-10, mean |error| 2.2e-8, maximum 7.7e-8
// (degree 8: 1.5e-11 / 2.2e-8 / 7.4e-8; libm's expf: 3.5e-11 / 2.1e-8).
__device__ __forceinline__ f32x2 exp_nonpos_f32x2m(f32x2 d) {
  d.x = fmaxf(d.x, -80.0f);  // exp(-80) = 1.8e-35 does not register in a sum >= 1; also maps -inf masks
  d.y = fmaxf(d.y, -80.0f);
  const f32x2 magic = (f32x2)(12582912.0f);
  const f32x2 t = __builtin_elementwise_fma(d, (f32x2)(1.44269504088896340736f), magic);
  const f32x2 n = t - magic;
  f32x2 r = __builtin_elementwise_fma(n, (f32x2)(-0.693145751953125f), d);
  r = __builtin_elementwise_fma(n, (f32x2)(-1.42860682030941723212e-6f), r);
  f32x2 p = (f32x2)(1.98412698412698413e-04f);                              // 1/7!
  p = __builtin_elementwise_fma(p, r, (f32x2)(1.38888888888888889e-03f));   // 1/6!
  p = __builtin_elementwise_fma(p, r, (f32x2)(8.33333333333333333e-03f));   // 1/5!
  p = __builtin_elementwise_fma(p, r, (f32x2)(4.16666666666666667e-02f));   // 1/4!
  p = __builtin_elementwise_fma(p, r, (f32x2)(1.66666666666666667e-01f));   // 1/3!
  p = __builtin_elementwise_fma(p, r, (f32x2)(0.5f));
  p = __builtin_elementwise_fma(p, r, (f32x2)(1.0f));
  p = __builtin_elementwise_fma(p, r, (f32x2)(1.0f));
  f32x2 out;
  out.x = __uint_as_float(__float_as_uint(p.x) + (__float_as_uint(t.x) << 23));
  out.y = __uint_as_float(__float_as_uint(p.y) + (__float_as_uint(t.y) << 23));
  return out;
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_f32(float ident, float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(ident), __float_as_int(v), CTRL, ROW_MASK, 0xf, false));
}
// v_max3_f32 / v_max_f32_dpp by hand: fmaxf() makes the compiler quiet each operand first (v_max_f32 x, x, x), which doubles
// the instructions of a maximum over loaded values. NaNs need no care here: a row that holds one is recognised by its sum
// and handed to the per-row kernel.
__device__ __forceinline__ float min3_raw(float a, float b, float c) {
  float o;
  asm("v_min3_f32 %0, %1, %2, %3" : "=v"(o) : "v"(a), "v"(b), "v"(c));
  return o;
}
__device__ __forceinline__ float max3_raw(float a, float b, float c) {
  float o;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(o) : "v"(a), "v"(b), "v"(c));
  return o;
}
// The row maximum and the row sum across the wave: two DPP chains, step by step in ONE block. A DPP read needs two wait states
// after the VALU write of its source, and the compiler cannot see into the asm: a chain on its own pays `s_nop 1` in front of
// each of its six steps; here the other chain's step is one of the two states and `s_nop 0` the other -- 19 instructions for
// the two reductions instead of 31. (Lanes a DPP step has no source for keep their value: the destination is the second
// operand -- for the sum that is the compiler's own `v + dpp(0, v)`, whose lanes add +0: no partial sum here is -0, each
// starts from +0. The block ends one wait state after its last write: what a v_readlane of the result needs.)
#define CTC_MAX_SUM_DPP(CTRL) "v_max_f32_dpp %0, %0, %0 " CTRL "\n\tv_add_f32_dpp %1, %1, %1 " CTRL "\n\ts_nop 0\n\t"
__device__ __forceinline__ void wave_max_sum_f32(float& mx, float& sm) {
  asm volatile("s_nop 1\n\t"
               CTC_MAX_SUM_DPP("row_shr:1 row_mask:0xf bank_mask:0xf")
               CTC_MAX_SUM_DPP("row_shr:2 row_mask:0xf bank_mask:0xf")
               CTC_MAX_SUM_DPP("row_shr:4 row_mask:0xf bank_mask:0xf")
               CTC_MAX_SUM_DPP("row_shr:8 row_mask:0xf bank_mask:0xf")
               CTC_MAX_SUM_DPP("row_bcast:15 row_mask:0xa bank_mask:0xf")
               CTC_MAX_SUM_DPP("row_bcast:31 row_mask:0xc bank_mask:0xf")
               : "+v"(mx), "+v"(sm));
  mx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mx), 63));
  sm = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sm), 63));
}
#undef CTC_MAX_SUM_DPP
__device__ __forceinline__ float wave_sum_f32(float v) {
  v += dpp_f32<0x111, 0xf>(0.f, v);
  v += dpp_f32<0x112, 0xf>(0.f, v);
  v += dpp_f32<0x114, 0xf>(0.f, v);
  v += dpp_f32<0x118, 0xf>(0.f, v);
  v += dpp_f32<0x142, 0xa>(0.f, v);
  v += dpp_f32<0x143, 0xc>(0.f, v);
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ uint32_t lanes_below(uint64_t mask) {  // set bits of `mask` below this lane
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// one lane's 48 table slots, interleaved with the other lanes' (slot k of lane l at [k * 64 + l])
struct LaneTab {
  uint16_t* t;
  __device__ __forceinline__ uint16_t get(uint32_t k) const { return t[k * PF_ROWS]; }
  __device__ __forceinline__ void put(uint32_t k, uint16_t v) { t[k * PF_ROWS] = v; }
};

// DT: ctcdec_dtype of the rows -- 0 float32 (NC 16-byte loads of four labels per lane), 2 float16 / 3 bfloat16 (NC / 2 loads
// of eight labels, widened exactly to the same NC float4 groups: the arithmetic below never knows the difference)
// (native vector types: what a load returns stays in its registers untouched until the row is worked on -- and, unlike the HIP
//  vector classes, they can be read through a pointer with an address space)
typedef float PfF4 __attribute__((ext_vector_type(4)));
typedef uint32_t PfU4 __attribute__((ext_vector_type(4)));
template <int DT>
struct PfRaw {
  typedef PfF4 type;
};
template <>
struct PfRaw<2> {
  typedef PfU4 type;
};
template <>
struct PfRaw<3> {
  typedef PfU4 type;
};
template <int DT>
__device__ __forceinline__ float pf_widen(uint32_t h16) {
  return DT == 2 ? __half2float(__ushort_as_half((unsigned short)h16)) : __uint_as_float(h16 << 16);
}

// numpy's float32 exp (np_f32.h: np_exp_f32) for the arguments of a clean row's log-softmax, t = x - max <= 0 or -inf, without
// its special-case branches: the same operations in the same order, the underflow rule as a select (the clamp keeps the
// polynomial's inputs finite). For the four labels of a lane's group, two at a time in packed float32 instructions (v_pk_mul / add / fma_f32: each
// component rounds exactly like the scalar instruction; what has no packed form -- the maximum, the reciprocal, the scaling
// and the select -- stays scalar). A wave issues one vector instruction every ~5 cycles whatever it is (tools/micro/
// valu_rates.hip), so half the instructions is what counts. The division num / den is IEEE-exact in both forms:
//   default: the compiler's division (v_div_scale / v_rcp / four fused steps / v_div_fmas / v_div_fixup);
//   CTC_NP_SHORT_DIV: v_rcp + one Newton step + quotient + one fused correction -- den is in [0.8, 1.2] and num in [0.7, 1.5]
//   here, nothing needs scaling or fixing up; correct rounding of that sequence on THIS chip's v_rcp_f32 is checked for every
//   reduced argument by tools/micro/np_div_check.hip (round 6: 0 of 2.1e9 differ) before the macro may be set.
__device__ __forceinline__ f32x2 np_exp_nonpos_pk(f32x2 t) {
#pragma clang fp contract(off)
  f32x2 tc;
  tc.x = fmaxf(t.x, -104.0f);
  tc.y = fmaxf(t.y, -104.0f);
  const f32x2 magic = (f32x2)(12582912.0f);
  f32x2 q = tc * (f32x2)(1.442695040888963407359924681001892137f);
  q = q + magic;
  q = q - magic;
  f32x2 r = __builtin_elementwise_fma(q, (f32x2)(-6.93145752e-1f), tc);
  r = __builtin_elementwise_fma(q, (f32x2)(-1.42860677e-6f), r);
  f32x2 num = __builtin_elementwise_fma((f32x2)(5.082762527590693718096e-04f), r, (f32x2)(6.757896990527504603057e-03f));
  num = __builtin_elementwise_fma(num, r, (f32x2)(5.114512081637298353406e-02f));
  num = __builtin_elementwise_fma(num, r, (f32x2)(2.473615434895520810817e-01f));
  num = __builtin_elementwise_fma(num, r, (f32x2)(7.257664613233124478488e-01f));
  num = __builtin_elementwise_fma(num, r, (f32x2)(9.999999999980870924916e-01f));
  f32x2 den = __builtin_elementwise_fma((f32x2)(2.159509375685829852307e-02f), r, (f32x2)(-2.742335390411667452936e-01f));
  den = __builtin_elementwise_fma(den, r, (f32x2)(1.0f));
  f32x2 p;
#ifdef CTC_NP_SHORT_DIV
  f32x2 y0;
  y0.x = __builtin_amdgcn_rcpf(den.x);
  y0.y = __builtin_amdgcn_rcpf(den.y);
  const f32x2 e = __builtin_elementwise_fma(-den, y0, (f32x2)(1.0f));
  const f32x2 y = __builtin_elementwise_fma(e, y0, y0);
  const f32x2 q0 = num * y;
  const f32x2 rem = __builtin_elementwise_fma(-den, q0, num);
  p = __builtin_elementwise_fma(rem, y, q0);
#else
  p.x = num.x / den.x;
  p.y = num.y / den.y;
#endif
  f32x2 v;
  v.x = ldexpf(p.x, (int)q.x);
  v.y = ldexpf(p.y, (int)q.y);
  v.x = t.x <= -103.97208404541015625f ? 0.0f : v.x;
  v.y = t.y <= -103.97208404541015625f ? 0.0f : v.y;
  return v;
}
// ... and for rows all of whose arguments are in (-87, 0] -- every row of ordinary logits; a row that reaches further down is
// handed to the per-row kernel --: no clamp, no underflow select, and the scaling by 2^k as one integer add into the exponent
// field (the result is a normal number there: exactly what ldexpf gives; k sits in the low mantissa bits of q + 1.5 * 2^23).
// num / den, IEEE-exact: v_rcp_f32, quotient, one fused correction (den in [0.8, 1.2], num in [0.7, 1.5]: nothing to scale or
// fix up, and the reciprocal's 1 ulp is enough for the correction term). Checked against the compiler's division for EVERY
// reduced argument on this chip: tools/micro/np_div_check.hip, profiles/r06_np_div_check.txt -- 0 of 2 104 533 978 differ
// (with and without a Newton step on the reciprocal).
// N pairs at once, stage by stage. Why: on gfx950 a vector instruction that reads the result of the packed-float32
// instruction right before it costs a wait state, and the compiler -- which schedules one exponential's chain after the other --
// pays it with an `s_nop` between nearly every two instructions of the sixteen chains of a row (round 6: 102 of the 340
// instructions of a row's exponentials were s_nop, and a wave issues one instruction per ~5 cycles whatever it is). Written
// stage-major with the scheduler fenced between stages, consecutive instructions belong to different chains and nothing waits.
// Per element the operations of np_exp_nonpos_pk in the same order, less the clamp and the select: the same bits.
template <int N>
__device__ __forceinline__ void np_exp_nonpos_pk_fast_n(const f32x2 (&t)[N], f32x2 (&v)[N]) {
#pragma clang fp contract(off)
  const f32x2 magic = (f32x2)(12582912.0f);
  f32x2 q[N], qm[N], r[N], num[N], den[N], y0[N], q0[N];
#define CTC_STAGE(expr)                      \
  _Pragma("unroll") for (int i = 0; i < N; ++i) { expr; } \
  __builtin_amdgcn_sched_barrier(0);
  CTC_STAGE(q[i] = t[i] * (f32x2)(1.442695040888963407359924681001892137f))
  CTC_STAGE(qm[i] = q[i] + magic)
  CTC_STAGE(q[i] = qm[i] - magic)
  CTC_STAGE(r[i] = __builtin_elementwise_fma(q[i], (f32x2)(-6.93145752e-1f), t[i]))
  CTC_STAGE(r[i] = __builtin_elementwise_fma(q[i], (f32x2)(-1.42860677e-6f), r[i]))
  CTC_STAGE(num[i] = __builtin_elementwise_fma((f32x2)(5.082762527590693718096e-04f), r[i], (f32x2)(6.757896990527504603057e-03f));
            den[i] = __builtin_elementwise_fma((f32x2)(2.159509375685829852307e-02f), r[i], (f32x2)(-2.742335390411667452936e-01f)))
  CTC_STAGE(num[i] = __builtin_elementwise_fma(num[i], r[i], (f32x2)(5.114512081637298353406e-02f));
            den[i] = __builtin_elementwise_fma(den[i], r[i], (f32x2)(1.0f)))
  CTC_STAGE(num[i] = __builtin_elementwise_fma(num[i], r[i], (f32x2)(2.473615434895520810817e-01f));
            y0[i].x = __builtin_amdgcn_rcpf(den[i].x))
  CTC_STAGE(num[i] = __builtin_elementwise_fma(num[i], r[i], (f32x2)(7.257664613233124478488e-01f));
            y0[i].y = __builtin_amdgcn_rcpf(den[i].y))
  CTC_STAGE(num[i] = __builtin_elementwise_fma(num[i], r[i], (f32x2)(9.999999999980870924916e-01f)))
  CTC_STAGE(q0[i] = num[i] * y0[i])
  CTC_STAGE(num[i] = __builtin_elementwise_fma(-den[i], q0[i], num[i]))  // (the remainder)
  CTC_STAGE(q0[i] = __builtin_elementwise_fma(num[i], y0[i], q0[i]))
  CTC_STAGE(v[i].x = __uint_as_float(__float_as_uint(q0[i].x) + (__float_as_uint(qm[i].x) << 23));
            v[i].y = __uint_as_float(__float_as_uint(q0[i].y) + (__float_as_uint(qm[i].y) << 23)))
#undef CTC_STAGE
}
// index of element i of a row in the exchange buffer: eight floats of padding per 128 (the accumulator lanes of different
// leaves then read different banks)
__device__ __forceinline__ int np_pad(int i) { return i + ((i >> 7) << 3); }
constexpr size_t PF_TABS_BYTES = (size_t)PF_ROWS * SMALL_SET_SLOTS * 2;
// LDS a block needs beyond PF_LDS in numpy-order mode: the leaf sums of its 64 rows, and the exchange buffer of one row when it
// does not fit the set tables' bytes (which are idle during phase A)
__host__ __device__ inline size_t pf_np_rowbuf_bytes(int nc) { return ((size_t)(nc * 256 + nc * 16 + 16) * 4 + 15) & ~(size_t)15; }
__host__ __device__ inline size_t pf_np_extra_lds(int nc, int n_leaf) {
  const size_t ls = (size_t)n_leaf * PF_ROWS * 4;
  return ls + (pf_np_rowbuf_bytes(nc) <= PF_TABS_BYTES ? 0 : pf_np_rowbuf_bytes(nc));
}

// AL: rows start on 16-byte boundaries and hold a multiple of four (16-bit: eight) labels: 16-byte loads. !AL (float32 only):
// any label count and any 4-byte-aligned rows -- each lane fetches its four consecutive labels one by one (the common
// "1024 BPE pieces + blank = 1025 labels" shape); labels past the row's end read as -inf.
// NP (float32 rows): the sum of exponentials in the reference's own float32 arithmetic -- numpy's float32 exp per label, its
// pairwise summation order (np_sum.h) and, in phase B, its float32 log: a row's exponentials cross LDS once so that lane
// (leaf, j) adds the elements numpy's accumulator j of that leaf adds, in numpy's order; the leaf sums wait in LDS for phase B,
// where every lane combines its row's along the recursion's tree (a.np_prog). A frame's log-probabilities are then the
// reference's bits, and the decode of float32 logits equals the reference's to the last bit of every score.
template <int NC, int DT, bool AL = true, bool NP = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(NC <= 4 ? PF_WAVES : 1, NC <= 4 ? PF_WAVES : 8))) void frame_prune_fast(PruneArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x;
  const int64_t row_lo = a.row_base + (int64_t)blockIdx.x * PF_ROWS;
  const int64_t row_end = a.row_base + a.n_rows;
  if (row_lo >= row_end) return;
  // (wave-uniform, and said so: the 64-bit comparison goes through the vector unit, and everything counted against nrows --
  // the row loop, the rows' addresses -- would follow it there)
  const int nrows = __builtin_amdgcn_readfirstlane((int)(row_end - row_lo < (int64_t)PF_ROWS ? row_end - row_lo : (int64_t)PF_ROWS));
  uint16_t* ar_id = (uint16_t*)smem;                       // [PF_CAND][64 rows]
  float* ar_x = (float*)(smem + PF_LDS_IDS);               // [PF_CAND][64 rows]
  uint16_t* tabs = (uint16_t*)(smem + PF_LDS_IDS + PF_LDS_X);  // [SMALL_SET_SLOTS][64 rows]
  static_assert(!NP || DT == 0, "numpy-order sums: float32 rows");
  float* np_ls = (float*)(smem + PF_LDS);        // NP: [n_leaf][64 rows] leaf sums
  float* np_rb = pf_np_rowbuf_bytes(NC) <= PF_TABS_BYTES ? (float*)tabs : (float*)(smem + PF_LDS + (a.np_uniform8 ? 0 : (size_t)a.np_n_leaf * PF_ROWS * 4));
  constexpr bool WIDE = DT == 0;                 // float32 rows
  constexpr int NL = WIDE ? NC : NC / 2;         // 16-byte loads per lane and row
  constexpr int PER = WIDE ? 4 : 8;              // labels per load
  static_assert(WIDE || NC % 2 == 0, "16-bit rows: two float4 groups per load");
  static_assert(AL || WIDE, "element-wise loads: float32 rows only");
  typedef typename PfRaw<DT>::type Raw;
  const int V = a.n_labels;
  const int n4 = AL ? V / PER : (V + 3) / 4;     // loads (groups of four labels) per row
  const bool full_row = AL && n4 == NL * 64;     // every lane's loads lie inside the row (wave-uniform)
  const float tminf = (float)a.token_min_logp;
  // label id of element e of group k in this lane; is group k inside the row?
  auto id_of = [&](int k, int e) { return WIDE ? (k * 64 + lane) * 4 + e : ((k >> 1) * 64 + lane) * 8 + (k & 1) * 4 + e; };
  auto in_row = [&](int k) { return (WIDE ? k : (k >> 1)) * 64 + lane < n4; };

  // rows are walked in order: the utterance of the first one by bisection, the rest by stepping.
  // Round 5: the utterance bookkeeping is SCALAR (uniform loads from the constant address space: s_load, counted by lgkmcnt)
  // and the rows are read through a GLOBAL-address-space pointer. Until then the rows' base pointer -- fetched from the
  // per-utterance pointer array by a vector load -- made every row load a flat_load and put an unconditional
  // `s_waitcnt vmcnt(0)` in front of each row's arithmetic: the two rows "in flight" behind the one being worked on were waited
  // for the moment they were requested, and every row paid a full HBM round trip (3.8 TB/s at V = 1024, ~8 500 cycles a row).
  typedef const int64_t __attribute__((address_space(4))) * ConstI64;
  typedef const void* const __attribute__((address_space(4))) * ConstPtrs;
  typedef const Raw __attribute__((address_space(1))) * GlobalRaw;
  const ConstI64 row0_c = (ConstI64)a.utt_row0;
  const ConstPtrs logits_c = (ConstPtrs)a.utt_logits;
  // The bookkeeping is relative to the block: rows [.., u_end) of its 64 belong to utterance u, and u_row is the address the
  // block's row 0 would have inside that utterance -- a row's address is then one 32-bit multiply and a 64-bit add, and the
  // test for the next utterance a 32-bit compare (absolute 64-bit row numbers cost ~30 scalar instructions a row: the
  // 64-bit compares went through the vector unit, the product through three multiplies).
  const uint32_t row_bytes = (uint32_t)V * (WIDE ? 4u : 2u);
  auto rel_end = [&](int64_t r1) {
    return __builtin_amdgcn_readfirstlane((int)(r1 - row_lo < (int64_t)PF_ROWS ? r1 - row_lo : (int64_t)PF_ROWS));
  };
  int u = __builtin_amdgcn_readfirstlane(find_utt(a.utt_row0, a.n_utts, row_lo));
  int64_t u_r1 = row0_c[u + 1];
  int u_end = rel_end(u_r1);
  uint64_t u_row = (uint64_t)logits_c[u] + (uint64_t)(row_lo - row0_c[u]) * row_bytes;
  auto load_row = [&](int i, Raw(&r)[NL]) __attribute__((always_inline)) {  // i: the row's index in the block, never smaller than in the call before
    while (i >= u_end) {
      ++u;
      u_row = (uint64_t)logits_c[u] + (uint64_t)(row_lo - u_r1) * row_bytes;  // (u_r1: still the row this utterance starts at)
      u_r1 = row0_c[u + 1];
      u_end = rel_end(u_r1);
    }
    const GlobalRaw x4 = (GlobalRaw)(u_row + (uint64_t)((uint32_t)i * row_bytes));
    // Every load is UNCONDITIONAL (a lane past the row's end re-reads the row's first group; `widen` puts -inf there when the
    // row is worked on): a load behind a lane mask is a branch, and at the join the compiler can no longer count how many loads
    // are outstanding -- it waits for all of them, the prefetched rows included.
#pragma unroll
    for (int k = 0; k < NL; ++k) {
      const int i4 = k * 64 + lane;
      if constexpr (!AL) {
        const float __attribute__((address_space(1)))* xf = (const float __attribute__((address_space(1)))*)x4;
        const int e0 = i4 * 4;
        Raw v;
        v.x = xf[e0 < V ? e0 : 0];
        v.y = xf[e0 + 1 < V ? e0 + 1 : 0];
        v.z = xf[e0 + 2 < V ? e0 + 2 : 0];
        v.w = xf[e0 + 3 < V ? e0 + 3 : 0];
        r[k] = v;
      } else {
        r[k] = x4[i4 < n4 ? i4 : 0];
      }
    }
  };
  // FULL (here and in phase_a): every lane's loads lie inside the row -- 1024 labels in four loads, the usual shape. Compiled
  // apart from the rows that end inside a load, not tested per row: such a row has no lanes to mask, and where the two cases
  // meet again the compiler no longer keeps a row in the registers its loads wrote (adjacent pairs, as the packed instructions
  // want them) -- it paid sixteen selects and two dozen moves per row for a mask that is all ones.
  auto widen = [&](auto full_c, const Raw(&raw)[NL], float4(&r)[NC]) __attribute__((always_inline)) {
    constexpr bool FULL = decltype(full_c)::value;
    const float ninf = -INFINITY;
    if constexpr (WIDE) {
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        r[k] = make_float4(raw[k].x, raw[k].y, raw[k].z, raw[k].w);
        if constexpr (!AL) {  // labels past the end of the row
          const int e0 = (k * 64 + lane) * 4;
          if (e0 >= V) r[k].x = ninf;
          if (e0 + 1 >= V) r[k].y = ninf;
          if (e0 + 2 >= V) r[k].z = ninf;
          if (e0 + 3 >= V) r[k].w = ninf;
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < NL; ++k) {
        r[2 * k] = make_float4(pf_widen<DT>(raw[k].x & 0xFFFFu), pf_widen<DT>(raw[k].x >> 16), pf_widen<DT>(raw[k].y & 0xFFFFu),
                               pf_widen<DT>(raw[k].y >> 16));
        r[2 * k + 1] = make_float4(pf_widen<DT>(raw[k].z & 0xFFFFu), pf_widen<DT>(raw[k].z >> 16), pf_widen<DT>(raw[k].w & 0xFFFFu),
                                   pf_widen<DT>(raw[k].w >> 16));
      }
    }
    if constexpr (AL && !FULL) {  // lanes past the end of the row
#pragma unroll
      for (int k = 0; k < NC; ++k)
        if (!in_row(k)) r[k] = make_float4(ninf, ninf, ninf, ninf);
    }
  };

  // what phase A leaves for row i, in lane i
  float my_m = 0.f, my_rs = 0.f, my_s32 = 1.0f;
  double my_s = 1.0;
  int my_first = 0;
  uint32_t my_cnt = 0;

  // numpy's accumulators over the exchange buffer of row i (NP): lane (leaf, j) adds the elements accumulator j of that leaf
  // adds, in numpy's order; the leaf sums go to LDS for phase B. The leaves of the first sweep are fetched once per block.
  int np_off0 = 0, np_len0 = 0;
  if constexpr (NP) {
    const int leaf = lane >> 3;
    if (leaf < a.np_n_leaf) {
      np_off0 = a.np_leaf[2 * leaf];
      np_len0 = a.np_leaf[2 * leaf + 1];
    }
  }
  auto np_accumulate = [&](int i) __attribute__((always_inline)) {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int g = lane >> 3, j = lane & 7;
    const int nl = a.np_n_leaf;
    for (int base = 0; base < nl; base += 8) {
      const int leaf = base + g;
      const bool mine = leaf < nl;
      int off = np_off0, len = np_len0;
      if (base > 0) {
        off = len = 0;
        if (mine) {
          off = a.np_leaf[2 * leaf];
          len = a.np_leaf[2 * leaf + 1];
        }
      }
      float res = 0.f;
      if (len == 128 && (off & 127) == 0) {  // (the usual leaf: sixteen terms per accumulator, constant offsets from one address)
        const float* q = np_rb + np_pad(off) + j;
        float t0 = q[0], t1 = q[8], t2 = q[16], t3 = q[24], t4 = q[32], t5 = q[40], t6 = q[48], t7 = q[56];
        float t8 = q[64], t9 = q[72], t10 = q[80], t11 = q[88], t12 = q[96], t13 = q[104], t14 = q[112], t15 = q[120];
        float rr = t0 + t1;
        rr = rr + t2; rr = rr + t3; rr = rr + t4; rr = rr + t5; rr = rr + t6; rr = rr + t7; rr = rr + t8;
        rr = rr + t9; rr = rr + t10; rr = rr + t11; rr = rr + t12; rr = rr + t13; rr = rr + t14; rr = rr + t15;
        res = rr;
      } else if (len >= 8) {
        const int body = len - (len & 7);
        float rr = np_rb[np_pad(off + j)];
        for (int t = 8; t < body; t += 8) rr = rr + np_rb[np_pad(off + t + j)];
        res = rr;
      }
      // ((r0+r1)+(r2+r3)) + ((r4+r5)+(r6+r7)) inside the group of eight lanes: additions commute, an xor butterfly is that tree
      res = res + dpp_f32<0xB1, 0xf>(0.f, res);   // quad_perm [1, 0, 3, 2]
      res = res + dpp_f32<0x4E, 0xf>(0.f, res);   // quad_perm [2, 3, 0, 1]
      res = res + dpp_f32<0x141, 0xf>(0.f, res);  // row_half_mirror (both quads hold their sums in every lane by now)
      if ((len & 7) != 0 || len < 8) {  // leftovers (and leaves shorter than eight: a plain loop from 0), one by one
        const int body = len >= 8 ? len - (len & 7) : 0;
        if (len < 8) res = 0.f;
        for (int t = body; t < len; ++t) res = res + np_rb[np_pad(off + t)];
      }
      if (mine && j == 0) np_ls[leaf * PF_ROWS + i] = res;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();  // (the next row's exponentials go to the same buffer)
  };
  // The same for rows of one, two, four or eight leaves of 128 (a.np_uniform8: 1024 labels among them) with nothing left to
  // decide per row: one sweep, leaf g at element 128 g, sixteen terms per accumulator from an address that depends on the lane
  // alone (computed once per block; the per-term part is the instruction's offset), the eight leaf sums combined in registers
  // and the row's sum left in lane i. The additions and their order are np_accumulate's.
  const float* np_q8 = np_rb + np_pad(np_off0) + (lane & 7);
  auto np_accumulate8 = [&](int i) __attribute__((always_inline)) {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const float* q = np_q8;
    float t0 = q[0], t1 = q[8], t2 = q[16], t3 = q[24], t4 = q[32], t5 = q[40], t6 = q[48], t7 = q[56];
    float t8 = q[64], t9 = q[72], t10 = q[80], t11 = q[88], t12 = q[96], t13 = q[104], t14 = q[112], t15 = q[120];
    float rr = t0 + t1;
    rr = rr + t2; rr = rr + t3; rr = rr + t4; rr = rr + t5; rr = rr + t6; rr = rr + t7; rr = rr + t8;
    rr = rr + t9; rr = rr + t10; rr = rr + t11; rr = rr + t12; rr = rr + t13; rr = rr + t14; rr = rr + t15;
    float res = rr;
    res = res + dpp_f32<0xB1, 0xf>(0.f, res);   // quad_perm [1, 0, 3, 2]
    res = res + dpp_f32<0x4E, 0xf>(0.f, res);   // quad_perm [2, 3, 0, 1]
    res = res + dpp_f32<0x141, 0xf>(0.f, res);  // row_half_mirror
    if (a.np_n_leaf < 8) res = np_len0 != 0 ? res : 0.f;  // (groups of eight lanes without a leaf: what they read is not theirs)
    // every lane of a group holds its leaf's sum: numpy's tree ((S0+S1)+(S2+S3)) + ((S4+S5)+(S6+S7)) by three cross-lane
    // additions -- partners 8 lanes apart inside a row of sixteen, then rows 0 -> 1 and 2 -> 3, then row 1 -> row 3 (additions
    // commute) -- and the row's sum lands in lane i's register: no leaf sums in LDS, which buys the block's two further waves
    // per CU back
    float t = res + dpp_f32<0x128, 0xf>(0.f, res);  // row_ror:8
    t = t + dpp_f32<0x142, 0xa>(0.f, t);              // row_bcast:15 into rows 1 and 3
    t = t + dpp_f32<0x143, 0xc>(0.f, t);              // row_bcast:31 into rows 2 and 3
    const float total = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t), 63));
    if (lane == i) my_s32 = total;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();  // (the next row's exponentials go to the same buffer)
  };

  auto phase_a = [&](auto full_c, int i, const Raw(&raw)[NL]) __attribute__((always_inline)) -> uint32_t {
    constexpr bool FULL = decltype(full_c)::value;
    float4 r[NC];
    widen(full_c, raw, r);
    float mf = -INFINITY, rsf;
#pragma unroll
    for (int k = 0; k < NC; ++k) mf = max3_raw(max3_raw(mf, r[k].x, r[k].y), r[k].z, r[k].w);
    if (!AL) {  // (labels past the end of the row hold -inf for the maximum: nothing for the sum)
      rsf = 0.f;
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        const int e0 = (k * 64 + lane) * 4;
        rsf += ((e0 < V ? r[k].x : 0.f) + (e0 + 1 < V ? r[k].y : 0.f)) + ((e0 + 2 < V ? r[k].z : 0.f) + (e0 + 3 < V ? r[k].w : 0.f));
      }
    } else if (FULL) {  // (see prune_row_f32x4 on this sum)
      f32x2 rs2 = (f32x2)(0.f);
#pragma unroll
      for (int k = 0; k < NC; ++k) rs2 += (f32x2){r[k].x, r[k].y} + (f32x2){r[k].z, r[k].w};
      rsf = rs2.x + rs2.y;
    } else {  // lanes past the row hold -inf for the maximum: nothing for the sum
      rsf = 0.f;
#pragma unroll
      for (int k = 0; k < NC; ++k) rsf += in_row(k) ? (r[k].x + r[k].y) + (r[k].z + r[k].w) : 0.f;
    }
    wave_max_sum_f32(mf, rsf);
    const float m = mf, rs = rsf;
    uint32_t cnt = 0xFFFFu;  // "not a clean row": the per-row kernel takes it
    int first = 0;
    double s = 1.0;
    bool clean = isfinite(m) && rs == rs;
    if constexpr (NP) {
      // numpy-order sums: a row whose smallest logit is 87 or more below its maximum (exponentials that are denormal or zero in
      // float32; -inf masks; labels past the row's end do not count) takes the per-row kernel, whose exponential has the
      // underflow rules -- the 16 exponentials below then need neither a clamp nor a select, and scale by an integer add
      float lo = INFINITY;
      if constexpr (FULL) {
#pragma unroll
        for (int k = 0; k < NC; ++k) lo = min3_raw(min3_raw(lo, r[k].x, r[k].y), r[k].z, r[k].w);
      } else {
#pragma unroll
        for (int k = 0; k < NC; ++k) {
          if constexpr (AL) {
            if (in_row(k)) lo = min3_raw(min3_raw(lo, r[k].x, r[k].y), r[k].z, r[k].w);
          } else {
            const int e0 = (k * 64 + lane) * 4;
            lo = fminf(lo, fminf(fminf(e0 < V ? r[k].x : lo, e0 + 1 < V ? r[k].y : lo), fminf(e0 + 2 < V ? r[k].z : lo, e0 + 3 < V ? r[k].w : lo)));
          }
        }
      }
      if (clean && __ballot(!(lo - m > -87.0f)) != 0ull) clean = false;
    }
    if (clean) {
      if constexpr (NP) {
        // numpy's float32 exp of every label, in place, into the exchange buffer; their sum in any order for the screen (the
        // exact one -- numpy's accumulators, np_accumulate below -- is taken AFTER the screen: the wave issues in order, so the
        // screen's work stands between the LDS writes here and the reads there instead of a wait)
        f32x2 approx = (f32x2)(0.f);
        const f32x2 mm2 = (f32x2)(m);
        // (the exponentials of NP_IL groups of four labels at a time, stage by stage: np_exp_nonpos_pk_fast_n)
        constexpr int IL = NC % NP_IL == 0 ? NP_IL : 1;
        f32x2 ex[NC][2];
#pragma unroll
        for (int k0 = 0; k0 < NC; k0 += IL) {
          f32x2 tin[2 * IL], tout[2 * IL];
#pragma unroll
          for (int j = 0; j < IL; ++j) {
            tin[2 * j] = (f32x2){r[k0 + j].x, r[k0 + j].y} - mm2;
            tin[2 * j + 1] = (f32x2){r[k0 + j].z, r[k0 + j].w} - mm2;
          }
          np_exp_nonpos_pk_fast_n<2 * IL>(tin, tout);
#pragma unroll
          for (int j = 0; j < IL; ++j) {
            ex[k0 + j][0] = tout[2 * j];
            ex[k0 + j][1] = tout[2 * j + 1];
          }
        }
#pragma unroll
        for (int k = 0; k < NC; ++k)
          *(float4*)(np_rb + np_pad((k * 64 + lane) * 4)) = make_float4(ex[k][0].x, ex[k][0].y, ex[k][1].x, ex[k][1].y);
        if constexpr (FULL) {
#pragma unroll
          for (int k = 0; k < NC; ++k) approx += ex[k][0] + ex[k][1];
        } else {
#pragma unroll
          for (int k = 0; k < NC; ++k) {
            bool inside;  // (labels past the row's end hold -inf: garbage here, never read by the leaves, kept out of the screen's sum)
            if constexpr (AL) inside = in_row(k);
            else inside = (k * 64 + lane) * 4 + 3 < V;
            if (inside) approx += ex[k][0] + ex[k][1];
          }
        }
        s = (double)wave_sum_f32(approx.x + approx.y);
      } else {
      // sum of exponentials: float32 per lane (16 terms), fp64 across the lanes
      f32x2 acc = (f32x2)(0.f);
      const f32x2 mm = (f32x2)(m);
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        acc += exp_nonpos_f32x2m((f32x2){r[k].x, r[k].y} - mm);
        acc += exp_nonpos_f32x2m((f32x2){r[k].z, r[k].w} - mm);
      }
      s = wave_sum((double)(acc.x + acc.y));
      }
      // candidates: a float32 screen that cannot miss a survivor -- the threshold on the logits from a float32 logarithm
      // (|error| < 1e-6 (1 + lse)), lowered by a margin two orders above that and above the rounding of the sum. The sum is in
      // [1, 4096): v_log_f32 and one multiply (__logf guards denormal arguments with a dozen instructions more)
      const float xthr = (m + __builtin_amdgcn_logf((float)s) * 0.693147180559945309f) + tminf;
      const float pre = xthr - 3e-5f * (4.0f + fabsf(xthr));
      cnt = 0;
#pragma unroll
      for (int k = 0; k < NC; ++k) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float x = e == 0 ? r[k].x : e == 1 ? r[k].y : e == 2 ? r[k].z : r[k].w;
          const bool c = x >= pre;
          const uint64_t mk = __ballot(c);
          if (mk) {
            const uint32_t pos = cnt + lanes_below(mk);
            if (c && pos < (uint32_t)PF_CAND) {
              ar_id[pos * PF_ROWS + i] = (uint16_t)id_of(k, e);
              ar_x[pos * PF_ROWS + i] = x;
            }
            cnt += (uint32_t)__popcll(mk);
          }
        }
      }
      // the first maximum (numpy.argmax): when the maximum passes the screen, every label that ties for it is among the
      // candidates and phase B picks the smallest id; only a row whose maximum is below the threshold is searched here,
      // from the lane masks of `== m`
      if (cnt == 0) {
        first = 0x7FFFFFFF;
#pragma unroll
        for (int k = 0; k < NC; ++k) {
          if (first == 0x7FFFFFFF || (!WIDE && (k & 1))) {
            const uint64_t b0 = __ballot(r[k].x == m), b1 = __ballot(r[k].y == m), b2 = __ballot(r[k].z == m),
                           b3 = __ballot(r[k].w == m);
            const uint64_t any = b0 | b1 | b2 | b3;
            if (any) {
              const int l = __builtin_ctzll(any);
              const int e = ((b0 >> l) & 1ull) ? 0 : ((b1 >> l) & 1ull) ? 1 : ((b2 >> l) & 1ull) ? 2 : 3;
              // (16-bit rows: groups 2j and 2j+1 hold labels 8l..8l+3 and 8l+4..8l+7 of lane l -- the smaller id may
              // sit in the odd group of an earlier lane, so both groups of a load are looked at before the answer stands)
              const int cand = WIDE ? (k * 64 + l) * 4 + e : ((k >> 1) * 64 + l) * 8 + (k & 1) * 4 + e;
              if (cand < first) first = cand;
            }
          }
        }
      }
      if constexpr (NP) {
        if (a.np_uniform8) np_accumulate8(i);
        else np_accumulate(i);
      }
    }
    if (lane == i) {
      my_m = m;
      my_rs = rs;
      if constexpr (!NP) my_s = s;
      my_first = first;
      my_cnt = cnt;
    }
    return cnt;  // (wave-uniform)
  };

  // Rows in flight behind the one being worked on. EVERY iteration issues the same loads whatever the block's length (past its
  // end the last row is requested again: an L2 hit nobody looks at): the compiler places `s_waitcnt vmcnt(n)` by counting the
  // loads outstanding on every path into a block and keeping the SMALLEST count, so a single path that skips a row's loads
  // (a short block, the loop's last iterations) turned every wait into "all of them" -- the prefetch existed in the source only.
  auto row_at = [&](int i) { return i < nrows - 1 ? i : nrows - 1; };
  auto rows = [&](auto full_c) __attribute__((always_inline)) {
    if constexpr (NC <= 4) {
      // two rows in flight (three register buffers in rotation): at 13 waves per CU (LDS) and 4 KB a row that is ~100 KB per CU
      // on its way, what ~6 TB/s times the loaded memory latency asks for
      Raw ra[NL], rb[NL], rc[NL];
      load_row(row_at(0), ra);
      load_row(row_at(1), rb);
      for (int i = 0; i < nrows; i += 3) {
        load_row(row_at(i + 2), rc);
        phase_a(full_c, i, ra);
        load_row(row_at(i + 3), ra);
        if (i + 1 < nrows) phase_a(full_c, i + 1, rb);
        load_row(row_at(i + 4), rb);
        if (i + 2 < nrows) phase_a(full_c, i + 2, rc);
      }
    } else if constexpr (NC <= 8) {
      Raw ra[NL], rb[NL];
      load_row(row_at(0), ra);
      for (int i = 0; i < nrows; i += 2) {
        load_row(row_at(i + 1), rb);
        phase_a(full_c, i, ra);
        load_row(row_at(i + 2), ra);
        if (i + 1 < nrows) phase_a(full_c, i + 1, rb);
      }
    } else {
      // 2049 .. 4095 labels (round 5): a row is up to 64 registers per lane, there is no room for a second one in flight --
      // the other waves of the CU cover the wait (round 5 measured what the rows in flight are worth at V = 1024: 4 %)
      Raw ra[NL];
      for (int i = 0; i < nrows; ++i) {
        load_row(row_at(i), ra);
        phase_a(full_c, i, ra);
      }
    }
  };
  if constexpr (AL) {
    if (full_row) rows(std::true_type());
    else rows(std::false_type());
  } else {
    rows(std::false_type());
  }
  __syncthreads();  // (one wave: orders phase A's LDS writes before phase B's reads)

  // ---- phase B: lane = row
  const int64_t row = row_lo + lane;
  const uint32_t ms = (uint32_t)a.max_surv;
  bool slow = false;
  if (lane < nrows) {
    const uint32_t cnt = my_cnt;
    slow = cnt > (uint32_t)PF_CAND;
    if (!slow) {
      const double s = my_s;
      const double md = (double)my_m;
      double lse = 0.0;
      float l32 = 0.f;
      if constexpr (NP) {
        // this row's leaf sums, combined along numpy's recursion (every lane walks the same (dst, src) list on its own column)
        float s32 = my_s32;  // (up to eight leaves of 128: combined in registers by phase A)
        if (!a.np_uniform8) {
          for (int q = 0; q + 1 < a.np_n_leaf; ++q) {
            const int dst = a.np_prog[2 * q], src = a.np_prog[2 * q + 1];
            np_ls[dst * PF_ROWS + lane] = np_ls[dst * PF_ROWS + lane] + np_ls[src * PF_ROWS + lane];
          }
          s32 = np_ls[lane];
        }
        l32 = np_log_f32(s32);
      } else {
        lse = log_ge1(s);
      }
      auto logp_of = [&](float x) { return NP ? to_logp_np32(x, false, my_m, l32) : to_logp((double)x, false, md, lse); };
      const double best = logp_of(my_m);
      uint16_t* ids = ar_id + lane;
      float* xs = ar_x + lane;
      // the exact test (fp64, as in the per-row kernel) + insertion sort by id, in place
      uint32_t n = 0;
      uint32_t first = cnt > 0 ? 0xFFFFu : (uint32_t)my_first;  // (candidates: the smallest id whose logit is the maximum)
      for (uint32_t j = 0; j < cnt; ++j) {
        const uint16_t id = ids[j * PF_ROWS];
        const float x = xs[j * PF_ROWS];
        if (x == my_m && id < first) first = id;
        if (logp_of(x) >= a.token_min_logp) {
          uint32_t p = n;
          while (p > 0 && ids[(p - 1) * PF_ROWS] > id) {
            ids[p * PF_ROWS] = ids[(p - 1) * PF_ROWS];
            xs[p * PF_ROWS] = xs[(p - 1) * PF_ROWS];
            --p;
          }
          ids[p * PF_ROWS] = id;
          xs[p * PF_ROWS] = x;
          ++n;
        }
      }
      slow = n > SMALL_SET_MAX_KEYS || n >= ms;  // (n == ms with the argmax outside: the per-row kernel's overflow rules)
      if (!slow) {
        LaneTab tab{tabs + lane};
        const SmallSet r = small_set_order(tab, n, [ids](uint32_t k) { return (uint32_t)ids[k * PF_ROWS]; },
                                           first);
        uint16_t* out_id = a.surv_id + (size_t)row * ms;
        double* out_lp = a.surv_lp + (size_t)row * ms;
        uint32_t pos = 0;
        for (uint32_t k = 0; k <= r.mask; ++k) {
          const uint16_t v = tab.get(r.base + k);
          if (v != SMALL_SET_EMPTY) {
            const uint32_t pay = v >> SMALL_SET_ID_BITS;
            out_id[pos] = (uint16_t)(v & SMALL_SET_ID_MASK);
            out_lp[pos] = pay == SMALL_SET_ARGMAX ? best : logp_of(xs[pay * PF_ROWS]);
            ++pos;
          }
        }
        a.surv_cnt[row] = pos;
        a.row_sum[row] = (double)my_rs;
      }
    }
  }
  const uint64_t sm = __ballot(slow);
  if (sm) {
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(&a.overflow[3], (uint32_t)__popcll(sm));
    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
    if (slow) a.slow_rows[base + lanes_below(sm)] = (uint32_t)(row - a.row_base);
  }
}

// numpy's pairwise recursion over a row of V elements (np_sum.h): its leaves (offset, length) left to right and the additions
// that combine their sums, as (dst, src) leaf indices -- the result of a node lives where its leftmost leaf's did
struct NpPlan {
  int V = -1, n_leaf = 0, uniform8 = 0;
  uint16_t* d_leaf = nullptr;
  uint8_t* d_prog = nullptr;
};
static int np_plan_node(int off, int n, std::vector<uint16_t>& leaf, std::vector<uint8_t>& prog) {
  if (n <= 128) {
    leaf.push_back((uint16_t)off);
    leaf.push_back((uint16_t)n);
    return (int)leaf.size() / 2 - 1;
  }
  int n2 = n / 2;
  n2 -= n2 % 8;
  const int l = np_plan_node(off, n2, leaf, prog), r = np_plan_node(off + n2, n - n2, leaf, prog);
  prog.push_back((uint8_t)l);
  prog.push_back((uint8_t)r);
  return l;
}
static int np_plan_for(int V, hipStream_t stream, NpPlan** out, std::string* err) {
  static NpPlan plans[4];
  static int next = 0;
  for (NpPlan& p : plans)
    if (p.V == V) {
      *out = &p;
      return 0;
    }
  NpPlan& p = plans[next];
  next = (next + 1) % 4;
  std::vector<uint16_t> leaf;
  std::vector<uint8_t> prog;
  np_plan_node(0, V, leaf, prog);
  prog.push_back(0);  // (never empty)
  prog.push_back(0);
  HIP_TRY(hipStreamSynchronize(stream));  // (a launch in flight may still read the plan this one replaces)
  if (p.d_leaf) (void)hipFree(p.d_leaf);
  if (p.d_prog) (void)hipFree(p.d_prog);
  p.d_leaf = nullptr;
  p.d_prog = nullptr;
  p.V = -1;
  HIP_TRY(hipMalloc((void**)&p.d_leaf, leaf.size() * 2));
  HIP_TRY(hipMalloc((void**)&p.d_prog, prog.size()));
  HIP_TRY(hipMemcpy(p.d_leaf, leaf.data(), leaf.size() * 2, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(p.d_prog, prog.data(), prog.size(), hipMemcpyHostToDevice));
  p.n_leaf = (int)leaf.size() / 2;
  p.uniform8 = (p.n_leaf == 1 || p.n_leaf == 2 || p.n_leaf == 4 || p.n_leaf == 8) ? 1 : 0;
  for (size_t k = 0; k < leaf.size(); k += 2)
    if (leaf[k + 1] != 128 || (leaf[k] & 127) != 0) p.uniform8 = 0;
  p.V = V;
  *out = &p;
  return 0;
}

// ---- the launcher: prune_route.h decides, this launches what it names ------------------------------------------------------------
// f(std::integral_constant<int, NC>()) for the NC a route names: 1 .. 8, 12 or 16
template <class F>
static int with_nc(int nc, F f) {
  switch (nc) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 3: return f(std::integral_constant<int, 3>());
    case 4: return f(std::integral_constant<int, 4>());
    case 5: return f(std::integral_constant<int, 5>());
    case 6: return f(std::integral_constant<int, 6>());
    case 7: return f(std::integral_constant<int, 7>());
    case 8: return f(std::integral_constant<int, 8>());
    case 12: return f(std::integral_constant<int, 12>());
    default: return f(std::integral_constant<int, 16>());
  }
}
template <class F>
static int with_flag(bool b, F f) { return b ? f(std::true_type()) : f(std::false_type()); }
// a kernel with dynamic LDS: the attribute that allows its size, and the launch
template <class K, class... Args>
static int launch_lds(K kern, dim3 grid, dim3 block, size_t lds, hipStream_t stream, std::string* err, const Args&... args) {
  HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, grid, block, lds, stream, args...);
  return 0;
}

int launch_prune_on(const PruneArgs& a_in, hipStream_t stream, std::string* err) {
  PruneArgs a = a_in;
  const PruneRoute rt = prune_route(PruneShape{a.dtype, a.n_labels, a.rows_aligned4 != 0, a.rows_aligned16 != 0, a.pass,
                                               a.slow_rows != nullptr, a.n_rows, a.dense_hint != 0,
                                               prune_exp_of(getenv("CTCDEC_PRUNE_EXP")),
                                               prune_per_row_forced(getenv("CTCDEC_PRUNE_KERNEL"))});
  a.f32_np = rt.np ? 1 : 0;
  a.np_prog = nullptr;
  a.np_leaf = nullptr;
  a.np_n_leaf = 0;
  a.np_uniform8 = 0;
  if (a.n_rows > 0) {
    const uint32_t cap = set_table_cap((uint32_t)a.max_surv + 1);
    const size_t lds = prune_lds_bytes((size_t)a.max_surv, cap) * PRUNE_WAVES;
    if (lds > 160 * 1024) {
      if (err) *err = "token_min_logp admits too many labels per frame for the LDS set tables";
      return -1;
    }
    const dim3 grid((unsigned)((a.n_rows + PRUNE_WAVES - 1) / PRUNE_WAVES)), block(PRUNE_WAVES * 64);  // a wave per row
    const dim3 fgrid((unsigned)((a.n_rows + PF_ROWS - 1) / PF_ROWS)), fblock(64);                      // 64 rows per wave
    const dim3 rest((unsigned)std::min<int64_t>((a.n_rows + PRUNE_WAVES - 1) / PRUNE_WAVES, 2048));   // the listed rows
    int rc = 0;
    switch (rt.kernel) {
      case PRUNE_FAST_F32: {
        size_t flds = PF_LDS;
        if (rt.np) {  // numpy's summation plan for rows of this length
          NpPlan* plan = nullptr;
          if (np_plan_for(a.n_labels, stream, &plan, err)) return -1;
          a.np_leaf = plan->d_leaf;
          a.np_prog = plan->d_prog;
          a.np_n_leaf = plan->n_leaf;
          a.np_uniform8 = plan->uniform8;
          flds += pf_np_extra_lds(rt.nc, plan->uniform8 ? 0 : plan->n_leaf);
        }
        rc = with_nc(rt.nc, [&](auto nc) { return with_flag(rt.al, [&](auto al) { return with_flag(rt.np, [&](auto np) {
          constexpr int NC = decltype(nc)::value;
          return launch_lds(frame_prune_fast<NC, 0, decltype(al)::value, decltype(np)::value>, fgrid, fblock, flds, stream, err, a);
        }); }); });
        if (rc) return rc;
        if (rt.listed == PRUNE_LISTED_F32X4) rc = with_nc(rt.nc, [&](auto nc) {
          constexpr int NC = decltype(nc)::value <= 4 ? decltype(nc)::value : 4;
          return launch_lds(frame_prune_f32x4_listed<NC>, rest, block, lds, stream, err, a, cap);
        });
        else rc = launch_lds(frame_prune_listed<float>, rest, block, lds, stream, err, a, cap);
        break;
      }
      case PRUNE_FAST_16:
        rc = with_flag(a.dtype == 2, [&](auto f16) { return with_flag(rt.nc == 2, [&](auto one_load) {
          constexpr int NC = decltype(one_load)::value ? 2 : 4, DT = decltype(f16)::value ? 2 : 3;
          hipLaunchKernelGGL((frame_prune_fast<NC, DT>), fgrid, fblock, PF_LDS, stream, a);  // (12 KiB of LDS: no attribute)
          return launch_lds(frame_prune_listed<std::conditional_t<DT == 2, half_bits, bf16_bits>>, rest, block, lds, stream, err, a, cap);
        }); });
        break;
      case PRUNE_ROW_F32X4:
        rc = with_nc(rt.nc, [&](auto nc) { return with_flag(rt.pk, [&](auto pk) {
          constexpr int NC = decltype(nc)::value <= 4 ? decltype(nc)::value : 4;
          return launch_lds(frame_prune_f32x4<NC, decltype(pk)::value>, grid, block, lds, stream, err, a, cap);
        }); });
        break;
      case PRUNE_ROW_GENERIC:
        if (a.dtype == 0) rc = launch_lds(frame_prune<float>, grid, block, lds, stream, err, a, cap);
        else if (a.dtype == 1) rc = launch_lds(frame_prune<double>, grid, block, lds, stream, err, a, cap);
        else if (a.dtype == 2) rc = launch_lds(frame_prune<half_bits>, grid, block, lds, stream, err, a, cap);
        else rc = launch_lds(frame_prune<bf16_bits>, grid, block, lds, stream, err, a, cap);
        break;
    }
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
  }
  if (a.n_utts > 0) {
    if (a.pass == 0) hipLaunchKernelGGL(utt_sniff, dim3((unsigned)a.n_utts), dim3(64), 0, stream, a);
    else hipLaunchKernelGGL(utt_recount, dim3((unsigned)a.n_utts), dim3(64), 0, stream, a);
    HIP_TRY(hipGetLastError());
  }
  return 0;
}

int launch_sniff_exact_on(const PruneArgs& a, hipStream_t stream, std::string* err) {
  if (a.n_utts > 0) {
    hipLaunchKernelGGL(utt_sniff_exact, dim3((unsigned)a.n_utts), dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
  }
  return 0;
}

}  // namespace be
}  // namespace ctc
