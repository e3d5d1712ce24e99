// ctc_align_hip.hip -- the transcript kernels on gfx950, bodies in ctc_align.h. A translation unit of its own.
//   row_lse, row_lse_max            G lanes per row; both fold with row_fold
//   ctc_viterbi                     a workgroup per utterance, score columns in LDS
//   ctc_viterbi_long                a workgroup of 1024 threads per utterance, score columns and checkpoints in device memory
//   ctc_forward, ctc_posteriors,    a workgroup per record, a group of four states per thread in registers
//   ctc_find, ctc_viterbi_gaps        (256 threads up to 511 labels, 1024 above)
//   ctc_forward_wave, ctc_find_wave a wavefront per record of at most 127 labels
//   ctc_grad_rows                   G threads per row of a dense ctc_posteriors launch's tables
//   row_argmax, row_lse_argmax      G lanes per row; both fold with row_fold_arg
//   greedy_collapse                 a wavefront per utterance
//   ctc_forward_ends, _wave_ends    ctc_forward / ctc_forward_wave that also store a prefix' end states per frame
//   ctc_prefix_extend, _finish      a workgroup per (chunk of prefixes, tile of 256 columns[, segment of frames]), a column per thread
//   ctc_prefix_fill                 -inf into the rows of the prefixes nothing was launched for
//   ctc_prefix_advance              (prefix sessions) a lane per child: its end states from its parent's
// The launchers share timed_launch (the event pair of the kernel's log and the launch's error), for_dtype and for_threads.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "backend.h"
#include "ctc_align.h"
#include "hip_try.h"

namespace ctc {
namespace be {

// ---------------------------------------------------------------------------------------------
// row_lse: G lanes per row (a whole wave for wide rows, 16 or 4 lanes for small vocabularies, so that a wave takes 4 or 16
// rows). Every logit is read once: a row that starts on a 16-byte boundary in 16-byte vectors (single elements for the
// V mod (16 / element size) left over), any other row element by element in the same grouping. A lane folds 16 values at a
// time into its running (max, sum of exp) pair -- one exp for the rescale, one per value -- and the lanes' pairs are merged
// by a butterfly of shuffles. 8 bytes out per row.
// ---------------------------------------------------------------------------------------------
template <int DT>
__device__ __forceinline__ void unpack16(const uint4 q, double* out) {
  if (DT == 0) {
    out[0] = (double)__uint_as_float(q.x);
    out[1] = (double)__uint_as_float(q.y);
    out[2] = (double)__uint_as_float(q.z);
    out[3] = (double)__uint_as_float(q.w);
  } else if (DT == 1) {
    out[0] = __hiloint2double((int)q.y, (int)q.x);
    out[1] = __hiloint2double((int)q.w, (int)q.z);
  } else {
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
    CTC_UNROLL
    for (int k = 0; k < 4; ++k) {
      const uint16_t lo = (uint16_t)(w[k] & 0xFFFFu), hi = (uint16_t)(w[k] >> 16);
      out[2 * k] = (double)(DT == 2 ? f16_bits_to_f32(lo) : bf16_bits_to_f32(lo));
      out[2 * k + 1] = (double)(DT == 2 ? f16_bits_to_f32(hi) : bf16_bits_to_f32(hi));
    }
  }
}

// One row's fold by its G lanes, lane l: the (max, sum of exp) pair of the row in every lane, or with MAX_ONLY the largest
// entry that is not a NaN alone, without an exponential (row_lse_max, for the rows of a probability-like utterance).
template <int G, int DT, bool MAX_ONLY>
__device__ __forceinline__ LseAcc row_fold(const char* p, int V, int l) {
  constexpr int ESZ = DT == 0 ? 4 : DT == 1 ? 8 : 2;      // bytes per element
  constexpr int EPV = 16 / ESZ;                           // elements per 16-byte vector
  constexpr int VPB = ALIGN_LSE_BLOCK / EPV;              // vectors per block of values
  // Which values a lane folds, and in which order, depends on the element index alone -- never on where the row lies in memory:
  // the same row gives the same bits whether it comes alone, inside a batch or out of a staging buffer.
  const bool vec = ((uintptr_t)p & 15u) == 0;
  const int nvec = V / EPV, tail = nvec * EPV;
  LseAcc acc = lse_empty();
  for (int i = tail + l; i < V; i += G) {
    const double v = align_load(p, DT, (size_t)i);
    if (MAX_ONLY) acc.m = v > acc.m ? v : acc.m;
    else lse_push(acc, v);
  }
  const uint4* pv = (const uint4*)p;
  for (int base = 0; base < nvec; base += G * VPB) {
    double v[ALIGN_LSE_BLOCK];
    CTC_UNROLL
    for (int j = 0; j < VPB; ++j) {
      const int i = base + j * G + l;  // (neighbouring lanes, neighbouring 16-byte groups)
      if (i >= nvec) {
        CTC_UNROLL
        for (int k = 0; k < EPV; ++k) v[j * EPV + k] = align_neg_inf();
      } else if (vec) {
        unpack16<DT>(pv[i], v + j * EPV);
      } else {
        CTC_UNROLL
        for (int k = 0; k < EPV; ++k) v[j * EPV + k] = align_load(p, DT, (size_t)i * EPV + (size_t)k);
      }
    }
    if (MAX_ONLY) {
      CTC_UNROLL
      for (int i = 0; i < ALIGN_LSE_BLOCK; ++i) acc.m = v[i] > acc.m ? v[i] : acc.m;
    } else {
      lse_push_block(acc, v);
    }
  }
  CTC_UNROLL
  for (int off = G / 2; off >= 1; off >>= 1) {
    LseAcc o;
    o.m = __shfl_xor(acc.m, off, G);
    o.s = __shfl_xor(acc.s, off, G);
    if (MAX_ONLY) acc.m = o.m > acc.m ? o.m : acc.m;
    else acc = lse_merge(acc, o);
  }
  return acc;
}

template <int G, int DT>
__global__ __launch_bounds__(256) void row_lse(RowLseArgs a) {
  constexpr int RPB = 256 / G;                            // rows per workgroup
  constexpr int ESZ = DT == 0 ? 4 : DT == 1 ? 8 : 2;
  const int64_t row = (int64_t)blockIdx.x * RPB + (int)(threadIdx.x / G);
  const int l = (int)(threadIdx.x % G);
  if (row >= a.n_rows) return;
  int lo = 0, hi = a.n_utts;  // utt_row0[lo] <= row < utt_row0[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.utt_row0[mid] <= row) lo = mid;
    else hi = mid;
  }
  if (a.utt_is_prob[lo]) return;  // (the whole group of lanes: `row` is theirs alone)
  const int V = a.n_labels;
  const char* p = (const char*)a.utt_logits[lo] + (size_t)(row - a.utt_row0[lo]) * (size_t)V * ESZ;
  const LseAcc acc = row_fold<G, DT, false>(p, V, l);
  if (l == 0) a.lse[row] = lse_value(acc);
}

// ---------------------------------------------------------------------------------------------
// ctc_viterbi: 256 threads per utterance, both score columns in LDS, one barrier per frame (ctc_align.h)
// ---------------------------------------------------------------------------------------------
struct AlignGpuCtx {
  int tid, nt;
  __device__ __forceinline__ void sync() { __syncthreads(); }
};

__global__ __launch_bounds__(ALIGN_THREADS) void ctc_viterbi(ViterbiArgs a) {
  extern __shared__ double align_cols[];
  AlignGpuCtx cx{(int)threadIdx.x, ALIGN_THREADS};
  ctc_viterbi_utt(cx, a.utts[blockIdx.x], a.n_labels, a.dtype, a.blank, a.fold, a.clip_lo, align_cols);
}

// ---------------------------------------------------------------------------------------------
// ctc_viterbi_long: 1024 threads per utterance -- sixteen waves on a compute unit, four per SIMD, so at most 128 VGPRs --, both
// score columns and the checkpoints in device memory, one barrier per frame. No workgroup waits for another (ctc_align.h)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ALIGN_LONG_THREADS) void ctc_viterbi_long(ViterbiLongArgs a) {
  AlignGpuCtx cx{(int)threadIdx.x, ALIGN_LONG_THREADS};
  ctc_viterbi_long_utt(cx, a.utts[blockIdx.x], a.n_labels, a.dtype, a.blank, a.fold, a.clip_lo);
}

// ---------------------------------------------------------------------------------------------
// ctc_forward: one workgroup per hypothesis, one group of four states per thread in registers (256 threads up to 511 labels,
// 1024 above), the groups' last states in two LDS columns, one barrier per frame. ctc_forward_wave: a wavefront per
// hypothesis of at most 127 labels, four to a workgroup that never synchronises; the neighbour's state by one fp64 shuffle
// per frame (ctc_align.h)
// ---------------------------------------------------------------------------------------------
struct ForwardGpuCtx {
  enum { GROUPS = 1 };
  int tid, nt;
  __device__ __forceinline__ void sync() { __syncthreads(); }
};
constexpr int FORWARD_THREADS_MAX = 1024;
static_assert(FORWARD_THREADS_MAX * ForwardGpuCtx::GROUPS >= FORWARD_MAX_GROUPS, "a thread per group of the longest target");

template <int NT, int DT>
__global__ __launch_bounds__(NT) void ctc_forward(ForwardArgs a) {
  extern __shared__ double forward_cols[];
  ForwardGpuCtx cx{(int)threadIdx.x, NT};
  ctc_forward_hyp<DT>(cx, a.hyps[blockIdx.x], a.n_labels, a.blank, a.clip_lo, forward_cols);
}

struct ForwardWaveCtx {
  int lane;
  __device__ __forceinline__ double up(double v) { return __shfl_up(v, 1, 64); }
};

constexpr int FORWARD_WAVES = ALIGN_THREADS / 64;  // hypotheses per workgroup of ctc_forward_wave

template <int DT>
__global__ __launch_bounds__(ALIGN_THREADS) void ctc_forward_wave(ForwardArgs a) {
  const int i = (int)blockIdx.x * FORWARD_WAVES + (int)(threadIdx.x >> 6);
  if (i >= a.n_hyps) return;  // (a whole wave: nothing in this kernel waits for another wave)
  ForwardWaveCtx cx{(int)(threadIdx.x & 63u)};
  ctc_forward_wave_hyp<DT>(cx, a.hyps[i], a.n_labels, a.blank, a.clip_lo);
}

// ---------------------------------------------------------------------------------------------
// ctc_posteriors: one workgroup per utterance, one group of four states per thread for both passes (256 threads up to 511
// labels, 1024 above); the forward pass leaves its states in the utterance's table, the backward pass turns them into
// posteriors in place (ctc_align.h)
// ---------------------------------------------------------------------------------------------
// (four waves per SIMD: what 1024 threads need to be resident at all, and the 256-thread kernel is held to the same 128 VGPRs)
template <int NT, int DT>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(4))) void ctc_posteriors(PosteriorsArgs a) {
  extern __shared__ double posteriors_cols[];
  ForwardGpuCtx cx{(int)threadIdx.x, NT};
  ctc_posteriors_utt<DT>(cx, a.utts[blockIdx.x], a.n_labels, a.blank, a.clip_lo, a.dense, posteriors_cols);
}

// ---------------------------------------------------------------------------------------------
// ctc_grad_rows: G threads per row (a workgroup for wide rows, a wave or 16 lanes for small vocabularies, so that a workgroup
// takes 4 or 16 rows); a thread keeps K of its entries and their shares of gamma in registers between the pass that sums M and
// the pass that writes (ctc_align.h). Every logit and every gamma is read once, every gradient entry is written once, in
// neighbouring lanes' neighbouring entries. The sums over a row's threads are butterflies of shuffles inside a wave and, for a
// workgroup, the four waves' parts through LDS in a fixed order: no atomics, the same bits wherever the row runs.
// ---------------------------------------------------------------------------------------------
template <int G, int K>
struct GradGpuCtx {
  enum { KEEP = K };
  int tid, nt;
  double* parts;  // [8] (G == 256): the waves' parts of the two sums of a row
  __device__ __forceinline__ double sum(double v, int slot) {
    constexpr int W = G < 64 ? G : 64;
    CTC_UNROLL
    for (int off = W / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, W);
    if (G <= 64) return v;
    double* p = parts + 4 * slot;
    if ((tid & 63) == 0) p[tid >> 6] = v;
    __syncthreads();
    return (p[0] + p[1]) + (p[2] + p[3]);
  }
};

template <int G, int K, int DT, class GT>
__global__ __launch_bounds__(ALIGN_THREADS) void ctc_grad_rows(GradRowsArgs a) {
  static_assert(G == 16 || G == 64 || G == ALIGN_THREADS, "a row's threads: part of a wave, a wave or the workgroup");
  constexpr int RPB = ALIGN_THREADS / G;  // rows per workgroup
  __shared__ double parts[8];
  const int64_t row = (int64_t)blockIdx.x * RPB + (int)(threadIdx.x / G);
  if (row >= a.n_rows) return;  // (the whole group of threads: `row` is theirs alone, and a workgroup's when it synchronises)
  int lo = 0, hi = a.n_utts;  // utts[lo].row_begin <= row < utts[hi].row_begin
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.utts[mid].row_begin <= row) lo = mid;
    else hi = mid;
  }
  const GradUtt u = a.utts[lo];
  GradGpuCtx<G, K> cx{(int)(threadIdx.x % G), G, parts};
  ctc_grad_row<DT, GT>(cx, u, (int)(row - u.row_begin), a.n_labels, a.blank, a.clip_lo);
}

// ---------------------------------------------------------------------------------------------
// ctc_find: one workgroup per phrase, one group of four states per thread in registers, scores and start frames (256 threads
// up to 511 labels, 1024 above), the groups' last states in two LDS columns of 12 bytes an entry, one barrier per frame.
// ctc_find_wave: a wavefront per phrase of at most 127 labels, four to a workgroup that never synchronises; the neighbour's
// state by one fp64 and one int32 shuffle per frame. In both, the thread that owns the last label writes the trace and its
// wavefront alone selects the hits from it (ctc_align.h)
// ---------------------------------------------------------------------------------------------
// What find_select asks of a wavefront: the windows taken so far live one to a lane.
struct FindSelectGpu {
  int lane_;
  int32_t hs = 0, he = 0;
  __device__ __forceinline__ int lane() const { return lane_; }
  __device__ __forceinline__ int lanes() const { return 64; }
  __device__ __forceinline__ bool any(bool b) const { return __any(b ? 1 : 0) != 0; }
  // (the trace: stored by one lane of this wave, loaded by all of them)
  __device__ __forceinline__ void publish() const { __threadfence_block(); }
  __device__ __forceinline__ void best(double& v, int& t, int& s) const {
    CTC_UNROLL
    for (int off = 32; off >= 1; off >>= 1) {
      const double ov = __shfl_xor(v, off, 64);
      const int ot = __shfl_xor(t, off, 64), os = __shfl_xor(s, off, 64);
      if (ov > v || (ov == v && ot < t)) v = ov, t = ot, s = os;
    }
  }
  __device__ __forceinline__ void put(int j, int32_t s, int32_t e) {
    if (lane_ == j) hs = s, he = e;
  }
  __device__ __forceinline__ void get(int j, int32_t* s, int32_t* e) const {
    *s = __shfl(hs, j, 64);
    *e = __shfl(he, j, 64);
  }
};
static_assert(FIND_MAX_HITS <= 64, "a lane per window taken");

struct FindGpuCtx : FindSelectGpu {
  enum { GROUPS = 1 };
  int tid, nt;
  __device__ __forceinline__ FindGpuCtx(int tid_, int nt_) : FindSelectGpu{tid_ & 63}, tid(tid_), nt(nt_) {}
  __device__ __forceinline__ void sync() { __syncthreads(); }
  __device__ __forceinline__ bool same_wave(int other_tid) const { return (tid >> 6) == (other_tid >> 6); }
};
static_assert(FORWARD_THREADS_MAX * FindGpuCtx::GROUPS >= find_chunks(ALIGN_MAX_LABELS), "a thread per group of the longest phrase");

template <int NT, int DT>
__global__ __launch_bounds__(NT) void ctc_find(FindArgs a) {
  extern __shared__ double find_cols[];
  FindGpuCtx cx((int)threadIdx.x, NT);
  ctc_find_phrase<DT>(cx, a.phrases[blockIdx.x], a.n_labels, a.blank, a.clip_lo, a.max_hits, a.min_logp, find_cols);
}

struct FindWaveCtx : FindSelectGpu {
  __device__ __forceinline__ explicit FindWaveCtx(int lane) : FindSelectGpu{lane} {}
  __device__ __forceinline__ double up(double v) const { return __shfl_up(v, 1, 64); }
  __device__ __forceinline__ int32_t up_i(int32_t v) const { return __shfl_up(v, 1, 64); }
};
static_assert(find_chunks(FIND_WAVE_MAX_LABELS) <= 64, "a lane per group");

template <int DT>
__global__ __launch_bounds__(ALIGN_THREADS) void ctc_find_wave(FindArgs a) {
  const int i = (int)blockIdx.x * FORWARD_WAVES + (int)(threadIdx.x >> 6);
  if (i >= a.n_phrases) return;  // (a whole wave: nothing in this kernel waits for another wave)
  FindWaveCtx cx((int)(threadIdx.x & 63u));
  ctc_find_wave_phrase<DT>(cx, a.phrases[i], a.n_labels, a.blank, a.clip_lo, a.max_hits, a.min_logp);
}

// ---------------------------------------------------------------------------------------------
// row_lse_max: row_lse that also stores the row's largest entry that is not a NaN -- the m its (max, sum of exp) pair ends
// with: a second 8 bytes per row, no new arithmetic. Both kernels fold a row with row_fold, so the log-sum-exp has row_lse's
// bits, wherever the row lies in memory. The rows of a probability-like utterance, which row_lse skips, take the same loads
// and a plain maximum, without an exponential. Every logit is still read once.
// ---------------------------------------------------------------------------------------------
template <int G, int DT>
__global__ __launch_bounds__(256) void row_lse_max(RowLseArgs a, double* rmax) {
  constexpr int RPB = 256 / G;                            // rows per workgroup
  constexpr int ESZ = DT == 0 ? 4 : DT == 1 ? 8 : 2;
  const int64_t row = (int64_t)blockIdx.x * RPB + (int)(threadIdx.x / G);
  const int l = (int)(threadIdx.x % G);
  if (row >= a.n_rows) return;
  int lo = 0, hi = a.n_utts;  // utt_row0[lo] <= row < utt_row0[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.utt_row0[mid] <= row) lo = mid;
    else hi = mid;
  }
  const int V = a.n_labels;
  const char* p = (const char*)a.utt_logits[lo] + (size_t)(row - a.utt_row0[lo]) * (size_t)V * ESZ;
  if (a.utt_is_prob[lo]) {  // (the whole group of lanes: `row` is theirs alone)
    const LseAcc acc = row_fold<G, DT, true>(p, V, l);
    if (l == 0) rmax[row] = acc.m;
    return;
  }
  const LseAcc acc = row_fold<G, DT, false>(p, V, l);
  if (l == 0) {
    a.lse[row] = lse_value(acc);
    rmax[row] = acc.m;
  }
}

// ---------------------------------------------------------------------------------------------
// ctc_viterbi_gaps: one workgroup per utterance, one group of four states per thread in registers (256 threads up to 511
// labels, 1024 above), the groups' last states in two LDS columns (at most 16 KB), one barrier and one byte of back-pointers
// per group and frame (ctc_align.h)
// ---------------------------------------------------------------------------------------------
template <int NT, int DT>
__global__ __launch_bounds__(NT) void ctc_viterbi_gaps(ViterbiGapsArgs a) {
  extern __shared__ double gaps_cols[];
  ForwardGpuCtx cx{(int)threadIdx.x, NT};
  ctc_viterbi_gaps_utt<DT>(cx, a.utts[blockIdx.x], a.n_labels, a.blank, a.fold, a.clip_lo, gaps_cols);
}

// ---------------------------------------------------------------------------------------------
// row_argmax, row_lse_argmax: every row's most probable label (ctc_align.h, "greedy_collapse"), in row_lse's row mapping and
// with row_lse's loads. A lane keeps (largest entry that is not a NaN, smallest index of it) and the lanes' pairs are merged
// by a butterfly of shuffles that compares (value, index): the label does not depend on which lane folded which entry.
//   row_argmax       compares alone -- no exponential, no logarithm -- in the row's own format (float for f16 / bf16): the
//                    largest logit of a row is its largest probability. ARGMAX_ROWS successive rows per group of lanes.
//   row_lse_argmax   row_lse_max that also stores the label: next to the pair a lane runs row_fold's accumulator through
//                    row_fold's operations in row_fold's order, so lse has row_lse's bits and rmax row_lse_max's.
// ---------------------------------------------------------------------------------------------
template <int DT, class VT>
__device__ __forceinline__ void unpack16_as(const uint4 q, VT* out) {
  if (DT == 0) {
    out[0] = (VT)__uint_as_float(q.x);
    out[1] = (VT)__uint_as_float(q.y);
    out[2] = (VT)__uint_as_float(q.z);
    out[3] = (VT)__uint_as_float(q.w);
  } else if (DT == 1) {
    out[0] = (VT)__hiloint2double((int)q.y, (int)q.x);
    out[1] = (VT)__hiloint2double((int)q.w, (int)q.z);
  } else {
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
    CTC_UNROLL
    for (int k = 0; k < 4; ++k) {
      const uint16_t lo = (uint16_t)(w[k] & 0xFFFFu), hi = (uint16_t)(w[k] >> 16);
      out[2 * k] = (VT)(DT == 2 ? f16_bits_to_f32(lo) : bf16_bits_to_f32(lo));
      out[2 * k + 1] = (VT)(DT == 2 ? f16_bits_to_f32(hi) : bf16_bits_to_f32(hi));
    }
  }
}
template <int DT, class VT>
__device__ __forceinline__ VT load_as(const char* p, size_t i) {
  if (DT == 0) return (VT)((const float*)p)[i];
  if (DT == 1) return (VT)((const double*)p)[i];
  const uint16_t h = ((const uint16_t*)p)[i];
  return (VT)(DT == 2 ? f16_bits_to_f32(h) : bf16_bits_to_f32(h));
}

enum { ARG_ONLY = 0, ARG_MAX = 1, ARG_LSE = 2 };  // what row_fold_arg keeps next to the label: nothing, row_fold<MAX_ONLY>'s or row_fold's accumulator

// One row's label by its G lanes, lane l: ARG_NONE for a row without an entry above -inf. With ARG_MAX / ARG_LSE `acc` ends
// as row_fold<G, DT, true / false> leaves it -- the same values through the same operations.
template <int G, int DT, int MODE>
__device__ __forceinline__ int32_t row_fold_arg(const char* p, int V, int l, LseAcc& acc) {
  typedef typename std::conditional<MODE == ARG_ONLY && DT != 1, float, double>::type VT;
  constexpr int ESZ = DT == 0 ? 4 : DT == 1 ? 8 : 2;      // bytes per element
  constexpr int EPV = 16 / ESZ;                           // elements per 16-byte vector
  constexpr int VPB = MODE == ARG_ONLY ? 4 : ALIGN_LSE_BLOCK / EPV;  // vectors per block of values (row_fold's where acc is kept)
  constexpr int BLOCK = VPB * EPV;
  const VT NEG = (VT)align_neg_inf();
  const bool vec = ((uintptr_t)p & 15u) == 0;
  const int nvec = V / EPV, tail = nvec * EPV;
  acc = lse_empty();
  // the left-over elements: the row's highest indices, ascending in a lane
  VT tv = NEG;
  int32_t ti = ARG_NONE;
  for (int i = tail + l; i < V; i += G) {
    const VT v = load_as<DT, VT>(p, (size_t)i);
    if (v > tv) tv = v, ti = i;
    if constexpr (MODE == ARG_MAX) acc.m = v > acc.m ? v : acc.m;
    else if constexpr (MODE == ARG_LSE) lse_push(acc, v);
  }
  // the vectors: ascending indices in a lane, all below the left-over ones
  VT bv = NEG;
  int32_t bi = ARG_NONE;
  const uint4* pv = (const uint4*)p;
  for (int base = 0; base < nvec; base += G * VPB) {
    VT v[BLOCK];
    CTC_UNROLL
    for (int j = 0; j < VPB; ++j) {
      const int i = base + j * G + l;  // (neighbouring lanes, neighbouring 16-byte groups)
      if (i >= nvec) {
        CTC_UNROLL
        for (int k = 0; k < EPV; ++k) v[j * EPV + k] = NEG;
      } else if (vec) {
        unpack16_as<DT, VT>(pv[i], v + j * EPV);
      } else {
        CTC_UNROLL
        for (int k = 0; k < EPV; ++k) v[j * EPV + k] = load_as<DT, VT>(p, (size_t)i * EPV + (size_t)k);
      }
    }
    if constexpr (MODE == ARG_ONLY) {
      CTC_UNROLL
      for (int j = 0; j < VPB; ++j) {
        const int i0 = (base + j * G + l) * EPV;
        CTC_UNROLL
        for (int k = 0; k < EPV; ++k)
          if (v[j * EPV + k] > bv) bv = v[j * EPV + k], bi = i0 + k;  // (a slot past the row holds -inf: never greater)
      }
    } else {
      // Next to the exponentials the index costs a branch per block: the block's maximum -- which lse_push_block forms
      // anyway -- seldom beats the lane's, and only then is the block searched, from its end, for the first entry equal to it.
      VT bm = NEG;
      CTC_UNROLL
      for (int i = 0; i < BLOCK; ++i) bm = v[i] > bm ? v[i] : bm;
      if (bm > bv) {
        bv = bm;
        CTC_UNROLL
        for (int j = VPB - 1; j >= 0; --j) {
          const int i0 = (base + j * G + l) * EPV;
          CTC_UNROLL
          for (int k = EPV - 1; k >= 0; --k)
            if (v[j * EPV + k] == bm) bi = i0 + k;
        }
      }
    }
    if constexpr (MODE == ARG_MAX) {
      CTC_UNROLL
      for (int i = 0; i < BLOCK; ++i) acc.m = v[i] > acc.m ? v[i] : acc.m;
    } else if constexpr (MODE == ARG_LSE) {
      lse_push_block(acc, v);
    }
  }
  arg_merge(bv, bi, tv, ti);
  CTC_UNROLL
  for (int off = G / 2; off >= 1; off >>= 1) {
    arg_merge(bv, bi, (VT)__shfl_xor(bv, off, G), (int32_t)__shfl_xor(bi, off, G));
    if constexpr (MODE != ARG_ONLY) {
      LseAcc o;
      o.m = __shfl_xor(acc.m, off, G);
      o.s = __shfl_xor(acc.s, off, G);
      if constexpr (MODE == ARG_MAX) acc.m = o.m > acc.m ? o.m : acc.m;
      else acc = lse_merge(acc, o);
    }
  }
  return bi;
}

// The utterance that holds `row`: utt_row0[lo] <= row < utt_row0[lo + 1]
__device__ __forceinline__ int row_utt(const int64_t* utt_row0, int n_utts, int64_t row) {
  int lo = 0, hi = n_utts;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (utt_row0[mid] <= row) lo = mid;
    else hi = mid;
  }
  return lo;
}

constexpr int ARGMAX_ROWS = 4;  // successive rows a group of lanes takes in row_argmax

template <int G, int DT>
__global__ __launch_bounds__(256) void row_argmax(RowLseArgs a, int32_t* arg, int blank) {
  constexpr int RPB = 256 / G;                            // groups of lanes per workgroup
  constexpr int ESZ = DT == 0 ? 4 : DT == 1 ? 8 : 2;
  const int64_t first = ((int64_t)blockIdx.x * RPB + (int)(threadIdx.x / G)) * ARGMAX_ROWS;
  const int l = (int)(threadIdx.x % G);
  if (first >= a.n_rows) return;  // (the whole group of lanes: its rows are theirs alone)
  const int V = a.n_labels;
  int u = row_utt(a.utt_row0, a.n_utts, first);
  for (int r = 0; r < ARGMAX_ROWS; ++r) {
    const int64_t row = first + r;
    if (row >= a.n_rows) return;
    while (row >= a.utt_row0[u + 1]) ++u;  // (row < n_rows = utt_row0[n_utts]: ends inside the array)
    const char* p = (const char*)a.utt_logits[u] + (size_t)(row - a.utt_row0[u]) * (size_t)V * ESZ;
    LseAcc unused;
    const int32_t i = row_fold_arg<G, DT, ARG_ONLY>(p, V, l, unused);
    if (l == 0) arg[row] = i == ARG_NONE ? blank : i;
  }
}

template <int G, int DT>
__global__ __launch_bounds__(256) void row_lse_argmax(RowLseArgs a, double* rmax, int32_t* arg, int blank) {
  constexpr int RPB = 256 / G;                            // rows per workgroup
  constexpr int ESZ = DT == 0 ? 4 : DT == 1 ? 8 : 2;
  const int64_t row = (int64_t)blockIdx.x * RPB + (int)(threadIdx.x / G);
  const int l = (int)(threadIdx.x % G);
  if (row >= a.n_rows) return;
  const int u = row_utt(a.utt_row0, a.n_utts, row);
  const int V = a.n_labels;
  const char* p = (const char*)a.utt_logits[u] + (size_t)(row - a.utt_row0[u]) * (size_t)V * ESZ;
  LseAcc acc;
  if (a.utt_is_prob[u]) {  // (the whole group of lanes: `row` is theirs alone)
    const int32_t i = row_fold_arg<G, DT, ARG_MAX>(p, V, l, acc);
    if (l == 0) {
      rmax[row] = acc.m;
      arg[row] = i == ARG_NONE ? blank : i;
    }
    return;
  }
  const int32_t i = row_fold_arg<G, DT, ARG_LSE>(p, V, l, acc);
  if (l == 0) {
    a.lse[row] = lse_value(acc);
    rmax[row] = acc.m;
    arg[row] = i == ARG_NONE ? blank : i;
  }
}

// ---------------------------------------------------------------------------------------------
// greedy_collapse: a wavefront per utterance, four to a workgroup that never synchronises; a step takes 64 frames, one to a
// lane. The neighbours' labels come by shuffles, a token's ordinal by the ballots of "a run starts / ends here"; no LDS, no
// atomics (ctc_align.h)
// ---------------------------------------------------------------------------------------------
struct GreedyWaveCtx {
  int lane_;
  __device__ __forceinline__ int lane() const { return lane_; }
  __device__ __forceinline__ int lanes() const { return 64; }
  __device__ __forceinline__ int32_t up(int32_t v) const { return __shfl_up(v, 1, 64); }
  __device__ __forceinline__ int32_t down(int32_t v) const { return __shfl_down(v, 1, 64); }
  __device__ __forceinline__ int32_t first(int32_t v) const { return __shfl(v, 0, 64); }
  __device__ __forceinline__ int32_t last(int32_t v) const { return __shfl(v, 63, 64); }
  __device__ __forceinline__ uint64_t ballot(bool b) const { return __ballot(b ? 1 : 0); }
  __device__ __forceinline__ void publish() const { __threadfence_block(); }
};

__global__ __launch_bounds__(ALIGN_THREADS) void greedy_collapse(GreedyArgs a) {
  const int u = (int)blockIdx.x * FORWARD_WAVES + (int)(threadIdx.x >> 6);
  if (u >= a.n_utts) return;  // (a whole wave: nothing in this kernel waits for another wave)
  GreedyWaveCtx cx{(int)(threadIdx.x & 63u)};
  greedy_collapse_utt(cx, a, u);
}

// ---------------------------------------------------------------------------------------------
// Prefix scores. ctc_forward_ends / ctc_forward_wave_ends: the forward kernels' bodies with ENDS, kernels of their own, so
// that ctc_forward and ctc_forward_wave keep their code. ctc_prefix_extend: blockIdx.x = chunk * tiles + tile (the tiles of
// a chunk next to each other: they read the same rows), blockIdx.y = the segment of a split launch. A thread owns one column;
// a row's 256 entries are one coalesced load, formed into exp(e) once for the chunk's prefixes, whose weights come from LDS
// (ctc_align.h). No atomics: a split launch leaves the segments' sums to ctc_prefix_finish.
// ---------------------------------------------------------------------------------------------
template <int NT, int DT>
__global__ __launch_bounds__(NT) void ctc_forward_ends(ForwardArgs a, const PrefixEnds* ends) {
  extern __shared__ double forward_ends_cols[];
  ForwardGpuCtx cx{(int)threadIdx.x, NT};
  ctc_forward_hyp<DT, true>(cx, a.hyps[blockIdx.x], a.n_labels, a.blank, a.clip_lo, forward_ends_cols, ends + blockIdx.x);
}

template <int DT>
__global__ __launch_bounds__(ALIGN_THREADS) void ctc_forward_wave_ends(ForwardArgs a, const PrefixEnds* ends) {
  const int i = (int)blockIdx.x * FORWARD_WAVES + (int)(threadIdx.x >> 6);
  if (i >= a.n_hyps) return;  // (a whole wave: nothing in this kernel waits for another wave)
  ForwardWaveCtx cx{(int)(threadIdx.x & 63u)};
  ctc_forward_wave_hyp<DT, true>(cx, a.hyps[i], a.n_labels, a.blank, a.clip_lo, ends + i);
}

static_assert(PREFIX_COLS == ALIGN_THREADS, "a column per thread");

template <int DT>
__global__ __launch_bounds__(PREFIX_COLS) void ctc_prefix_extend(PrefixExtendArgs a) {
  __shared__ double prefix_w[PREFIX_W_DOUBLES];
  const int tiles = prefix_tiles(a.n_labels);
  const int chunk = (int)(blockIdx.x / (unsigned)tiles), tile = (int)(blockIdx.x % (unsigned)tiles);
  const int nseg = prefix_segments(a.chunks[chunk].T);
  const int s0 = a.split ? (int)blockIdx.y : 0, s1 = a.split ? s0 + 1 : nseg;
  if (s0 >= nseg) return;  // (the whole workgroup)
  AlignGpuCtx cx{(int)threadIdx.x, PREFIX_COLS};
  ctc_prefix_extend_tile<DT>(cx, a, chunk, tile * PREFIX_COLS + (int)threadIdx.x, s0, s1, prefix_w);
}

__global__ __launch_bounds__(PREFIX_COLS) void ctc_prefix_finish(PrefixExtendArgs a) {
  const int tiles = prefix_tiles(a.n_labels);
  const int chunk = (int)(blockIdx.x / (unsigned)tiles), c = (int)(blockIdx.x % (unsigned)tiles) * PREFIX_COLS + (int)threadIdx.x;
  if (c < a.n_labels) ctc_prefix_finish_col(a, chunk, c);
}

// rows[blockIdx.y] of next[.][V]: -inf
__global__ __launch_bounds__(PREFIX_COLS) void ctc_prefix_fill(double* next, const int32_t* rows, int V) {
  const int c = (int)blockIdx.x * PREFIX_COLS + (int)threadIdx.x;
  if (c < V) next[(size_t)rows[blockIdx.y] * (size_t)V + (size_t)c] = align_neg_inf();
}

// ctc_prefix_advance (prefix sessions): a lane per child -- the recursion is two states wide --, a wavefront per workgroup so
// that a launch of a few hundred waves spreads over the compute units; the host orders the children by utterance. Vector
// loads and stores only, no LDS, no atomics (ctc_align.h).
template <int DT>
__global__ __launch_bounds__(PREFIX_ADVANCE_THREADS) void ctc_prefix_advance(PrefixAdvanceArgs a) {
  const int i = (int)blockIdx.x * PREFIX_ADVANCE_THREADS + (int)threadIdx.x;
  if (i < a.n_kids) ctc_prefix_advance_child<DT>(a.kids[i], a.n_labels, a.blank, a.clip_lo);
}

// ---------------------------------------------------------------------------------------------
// launches. Every launcher validates its arguments, then makes one timed_launch: the kernel's instantiation is picked by
// for_dtype (ctc_align.h) and, where the kernel has two sizes, for_threads; the row kernels' lanes per row by for_row_lanes.
// ---------------------------------------------------------------------------------------------
// kernel times: one pair of events per launch since the last reset, one log per kernel
struct EventLog {
  std::vector<hipEvent_t> ev;
  size_t used = 0;
  int next(hipEvent_t* out, std::string* err) {
    if (used == ev.size()) {
      hipEvent_t e;
      HIP_TRY(hipEventCreate(&e));
      ev.push_back(e);
    }
    *out = ev[used++];
    return 0;
  }
  double total() {
    double sum = 0.0;
    for (size_t k = 0; k + 1 < used; k += 2) {
      float ms = 0.f;
      if (hipEventSynchronize(ev[k + 1]) == hipSuccess && hipEventElapsedTime(&ms, ev[k], ev[k + 1]) == hipSuccess) sum += (double)ms;
    }
    return sum;
  }
};
static EventLog g_logs[ALIGN_KERNELS];

void align_timing_reset() {
  for (EventLog& log : g_logs) log.used = 0;
}
double align_kernel_ms(AlignKernel kind) { return g_logs[kind].total(); }
int align_kernel_launches(AlignKernel kind) { return (int)(g_logs[kind].used / 2); }

// launch() between two events of the kernel's log, and the error the launch left
template <class F>
static int timed_launch(AlignKernel kind, hipStream_t stream, std::string* err, F launch) {
  hipEvent_t e0, e1;
  if (g_logs[kind].next(&e0, err) || g_logs[kind].next(&e1, err)) return -1;
  HIP_TRY(hipEventRecord(e0, stream));
  launch();
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(e1, stream));
  return 0;
}
static int bad_launch(std::string* err, const char* what) {
  if (err) *err = what;
  return -1;
}

// f(std::integral_constant<int, NT>): 256 threads when every record of the launch has at most 256 groups of states, else 1024
template <class F>
static void for_threads(int max_chunks, F f) {
  if (max_chunks <= ALIGN_THREADS) f(std::integral_constant<int, ALIGN_THREADS>());
  else f(std::integral_constant<int, FORWARD_THREADS_MAX>());
}
// f(std::integral_constant<int, G>): the lanes per row of row_lse and row_lse_max, by the vocabulary alone -- the same
// grouping in both, so the same bits
template <class F>
static void for_row_lanes(int V, F f) {
  if (V >= 256) f(std::integral_constant<int, 64>());
  else if (V >= 32) f(std::integral_constant<int, 16>());
  else f(std::integral_constant<int, 4>());
}
template <int G>
static dim3 row_grid(int64_t n_rows) { return dim3((unsigned)((n_rows + (256 / G) - 1) / (256 / G))); }

int launch_row_lse_on(const RowLseArgs& a, hipStream_t stream, std::string* err) {
  if (a.n_rows <= 0 || a.n_utts <= 0) return 0;
  if (a.dtype < 0 || a.dtype > 3 || a.n_labels < 1 || a.n_rows > (int64_t)0x7FFFFFFF * 4) return bad_launch(err, "row_lse: bad arguments");
  return timed_launch(K_ROW_LSE, stream, err, [&] {
    for_row_lanes(a.n_labels, [&](auto g) {
      for_dtype(a.dtype, [&](auto dt) {
        constexpr int G = decltype(g)::value, DT = decltype(dt)::value;
        hipLaunchKernelGGL((row_lse<G, DT>), row_grid<G>(a.n_rows), dim3(256), 0, stream, a);
      });
    });
  });
}

int launch_row_lse_max_on(const RowLseArgs& a, double* rmax, hipStream_t stream, std::string* err) {
  if (a.n_rows <= 0 || a.n_utts <= 0) return 0;
  if (a.dtype < 0 || a.dtype > 3 || a.n_labels < 1 || a.n_rows > (int64_t)0x7FFFFFFF * 4 || !rmax)
    return bad_launch(err, "row_lse_max: bad arguments");
  return timed_launch(K_ROW_LSE_MAX, stream, err, [&] {
    for_row_lanes(a.n_labels, [&](auto g) {
      for_dtype(a.dtype, [&](auto dt) {
        constexpr int G = decltype(g)::value, DT = decltype(dt)::value;
        hipLaunchKernelGGL((row_lse_max<G, DT>), row_grid<G>(a.n_rows), dim3(256), 0, stream, a, rmax);
      });
    });
  });
}

// (ARGMAX_ROWS rows to a group of lanes)
int launch_row_argmax_on(const RowLseArgs& a, int32_t* arg, int blank, hipStream_t stream, std::string* err) {
  if (a.n_rows <= 0 || a.n_utts <= 0) return 0;
  if (a.dtype < 0 || a.dtype > 3 || a.n_labels < 1 || a.n_rows > (int64_t)0x7FFFFFFF * 4 || !arg || blank < 0 || blank >= a.n_labels)
    return bad_launch(err, "row_argmax: bad arguments");
  return timed_launch(K_ROW_ARGMAX, stream, err, [&] {
    for_row_lanes(a.n_labels, [&](auto g) {
      for_dtype(a.dtype, [&](auto dt) {
        constexpr int G = decltype(g)::value, DT = decltype(dt)::value;
        hipLaunchKernelGGL((row_argmax<G, DT>), row_grid<G>((a.n_rows + ARGMAX_ROWS - 1) / ARGMAX_ROWS), dim3(256), 0, stream, a, arg, blank);
      });
    });
  });
}

int launch_row_lse_argmax_on(const RowLseArgs& a, double* rmax, int32_t* arg, int blank, hipStream_t stream, std::string* err) {
  if (a.n_rows <= 0 || a.n_utts <= 0) return 0;
  if (a.dtype < 0 || a.dtype > 3 || a.n_labels < 1 || a.n_rows > (int64_t)0x7FFFFFFF * 4 || !rmax || !arg || blank < 0 || blank >= a.n_labels)
    return bad_launch(err, "row_lse_argmax: bad arguments");
  return timed_launch(K_ROW_LSE_ARGMAX, stream, err, [&] {
    for_row_lanes(a.n_labels, [&](auto g) {
      for_dtype(a.dtype, [&](auto dt) {
        constexpr int G = decltype(g)::value, DT = decltype(dt)::value;
        hipLaunchKernelGGL((row_lse_argmax<G, DT>), row_grid<G>(a.n_rows), dim3(256), 0, stream, a, rmax, arg, blank);
      });
    });
  });
}

int launch_greedy_collapse_on(const GreedyArgs& a, hipStream_t stream, std::string* err) {
  if (a.n_utts <= 0) return 0;
  if (!a.arg || !a.row0 || (a.write ? !a.tok_off || !a.label || !a.start || !a.end : !a.count) ||
      (a.write && a.fold && (!a.lse || !a.rmax || !a.is_prob || !a.logp || !a.score)))
    return bad_launch(err, "greedy_collapse: bad arguments");
  return timed_launch(K_GREEDY_COLLAPSE, stream, err, [&] {
    hipLaunchKernelGGL(greedy_collapse, dim3((unsigned)((a.n_utts + FORWARD_WAVES - 1) / FORWARD_WAVES)), dim3(ALIGN_THREADS), 0, stream, a);
  });
}

int launch_ctc_viterbi_on(const ViterbiArgs& a, hipStream_t stream, std::string* err) {
  if (a.n_utts <= 0) return 0;
  if (a.max_chunks < 1 || a.max_chunks > align_chunks(ALIGN_MAX_LABELS))
    return bad_launch(err, "ctc_viterbi: more states than two score columns in LDS hold");
  const size_t lds = (size_t)2 * 4 * (size_t)a.max_chunks * sizeof(double);  // <= 64 KB
  return timed_launch(K_VITERBI, stream, err, [&] {
    hipLaunchKernelGGL(ctc_viterbi, dim3((unsigned)a.n_utts), dim3(ALIGN_THREADS), lds, stream, a);
  });
}

int launch_ctc_viterbi_long_on(const ViterbiLongArgs& a, hipStream_t stream, std::string* err) {
  if (a.n_utts <= 0) return 0;
  if (a.dtype < 0 || a.dtype > 3 || !a.utts || a.n_labels < 1 || a.blank < 0 || a.blank >= a.n_labels)
    return bad_launch(err, "ctc_viterbi_long: bad arguments");
  return timed_launch(K_VITERBI_LONG, stream, err, [&] {
    hipLaunchKernelGGL(ctc_viterbi_long, dim3((unsigned)a.n_utts), dim3(ALIGN_LONG_THREADS), 0, stream, a);
  });
}

int launch_ctc_viterbi_gaps_on(const ViterbiGapsArgs& a, hipStream_t stream, std::string* err) {
  if (a.n_utts <= 0) return 0;
  if (a.dtype < 0 || a.dtype > 3 || a.max_chunks < 1 || a.max_chunks > align_chunks(ALIGN_MAX_LABELS))
    return bad_launch(err, "ctc_viterbi_gaps: more states than the kernel holds");
  const size_t lds = (size_t)2 * (size_t)a.max_chunks * sizeof(double);  // <= 16 KB
  return timed_launch(K_VITERBI_GAPS, stream, err, [&] {
    for_dtype(a.dtype, [&](auto dt) {
      for_threads(a.max_chunks, [&](auto nt) {
        constexpr int NT = decltype(nt)::value, DT = decltype(dt)::value;
        hipLaunchKernelGGL((ctc_viterbi_gaps<NT, DT>), dim3((unsigned)a.n_utts), dim3(NT), lds, stream, a);
      });
    });
  });
}

int launch_ctc_forward_on(const ForwardArgs& a, int wave, hipStream_t stream, std::string* err) {
  if (a.n_hyps <= 0) return 0;
  if (a.dtype < 0 || a.dtype > 3 || a.max_chunks < 1 || a.max_chunks > (wave ? align_chunks(FORWARD_WAVE_MAX_LABELS) : align_chunks(ALIGN_MAX_LABELS)))
    return bad_launch(err, "ctc_forward: more states than the kernel holds");
  const size_t lds = (size_t)2 * (size_t)a.max_chunks * sizeof(double);  // (ctc_forward) <= 16 KB
  return timed_launch(K_FORWARD, stream, err, [&] {
    for_dtype(a.dtype, [&](auto dt) {
      constexpr int DT = decltype(dt)::value;
      if (wave) {
        hipLaunchKernelGGL(ctc_forward_wave<DT>, dim3((unsigned)((a.n_hyps + FORWARD_WAVES - 1) / FORWARD_WAVES)), dim3(ALIGN_THREADS), 0, stream, a);
        return;
      }
      for_threads(a.max_chunks, [&](auto nt) {
        constexpr int NT = decltype(nt)::value;
        hipLaunchKernelGGL((ctc_forward<NT, DT>), dim3((unsigned)a.n_hyps), dim3(NT), lds, stream, a);
      });
    });
  });
}

int launch_ctc_forward_ends_on(const ForwardArgs& a, const PrefixEnds* ends, int wave, hipStream_t stream, std::string* err) {
  if (a.n_hyps <= 0) return 0;
  if (a.dtype < 0 || a.dtype > 3 || !ends || a.max_chunks < 1 ||
      a.max_chunks > (wave ? align_chunks(FORWARD_WAVE_MAX_LABELS) : align_chunks(ALIGN_MAX_LABELS)))
    return bad_launch(err, "ctc_forward_ends: more states than the kernel holds");
  const size_t lds = (size_t)2 * (size_t)a.max_chunks * sizeof(double);  // (ctc_forward_ends) <= 16 KB
  return timed_launch(K_FORWARD, stream, err, [&] {
    for_dtype(a.dtype, [&](auto dt) {
      constexpr int DT = decltype(dt)::value;
      if (wave) {
        hipLaunchKernelGGL(ctc_forward_wave_ends<DT>, dim3((unsigned)((a.n_hyps + FORWARD_WAVES - 1) / FORWARD_WAVES)), dim3(ALIGN_THREADS), 0, stream, a, ends);
        return;
      }
      for_threads(a.max_chunks, [&](auto nt) {
        constexpr int NT = decltype(nt)::value;
        hipLaunchKernelGGL((ctc_forward_ends<NT, DT>), dim3((unsigned)a.n_hyps), dim3(NT), lds, stream, a, ends);
      });
    });
  });
}

// ctc_prefix_extend and, for a split launch, ctc_prefix_finish behind it
int launch_ctc_prefix_extend_on(const PrefixExtendArgs& a, hipStream_t stream, std::string* err) {
  if (a.n_chunks <= 0) return 0;
  const int64_t blocks = (int64_t)a.n_chunks * prefix_tiles(a.n_labels);
  if (a.dtype < 0 || a.dtype > 3 || a.n_labels < 1 || a.blank < 0 || a.blank >= a.n_labels || a.max_segs < 1 || a.max_segs > 65535 ||
      blocks > (int64_t)0x7FFFFFFF || !a.chunks || !a.ends || !a.last || !a.next || (a.split && !a.partial))
    return bad_launch(err, "ctc_prefix_extend: bad arguments");
  const dim3 grid((unsigned)blocks, a.split ? (unsigned)a.max_segs : 1u);
  if (timed_launch(K_PREFIX_EXTEND, stream, err, [&] {
        for_dtype(a.dtype, [&](auto dt) {
          hipLaunchKernelGGL(ctc_prefix_extend<decltype(dt)::value>, grid, dim3(PREFIX_COLS), 0, stream, a);
        });
      }))
    return -1;
  if (!a.split) return 0;
  return timed_launch(K_PREFIX_EXTEND, stream, err, [&] {
    hipLaunchKernelGGL(ctc_prefix_finish, dim3((unsigned)blocks), dim3(PREFIX_COLS), 0, stream, a);
  });
}

int launch_ctc_prefix_fill_on(double* next, const int32_t* rows, int32_t n_rows, int32_t V, hipStream_t stream, std::string* err) {
  if (n_rows <= 0) return 0;
  if (!next || !rows || V < 1 || n_rows > 65535) return bad_launch(err, "ctc_prefix_fill: bad arguments");
  return timed_launch(K_PREFIX_EXTEND, stream, err, [&] {
    hipLaunchKernelGGL(ctc_prefix_fill, dim3((unsigned)prefix_tiles(V), (unsigned)n_rows), dim3(PREFIX_COLS), 0, stream, next, rows, V);
  });
}

int launch_ctc_prefix_advance_on(const PrefixAdvanceArgs& a, hipStream_t stream, std::string* err) {
  if (a.n_kids <= 0) return 0;
  if (a.dtype < 0 || a.dtype > 3 || a.n_labels < 1 || a.blank < 0 || a.blank >= a.n_labels || !a.kids)
    return bad_launch(err, "ctc_prefix_advance: bad arguments");
  const unsigned blocks = (unsigned)((a.n_kids + PREFIX_ADVANCE_THREADS - 1) / PREFIX_ADVANCE_THREADS);
  return timed_launch(K_PREFIX_ADVANCE, stream, err, [&] {
    for_dtype(a.dtype, [&](auto dt) {
      hipLaunchKernelGGL(ctc_prefix_advance<decltype(dt)::value>, dim3(blocks), dim3(PREFIX_ADVANCE_THREADS), 0, stream, a);
    });
  });
}

int launch_ctc_posteriors_on(const PosteriorsArgs& a, hipStream_t stream, std::string* err) {
  if (a.n_utts <= 0) return 0;
  if (a.dtype < 0 || a.dtype > 3 || a.max_chunks < 1 || a.max_chunks > align_chunks(ALIGN_MAX_LABELS))
    return bad_launch(err, "ctc_posteriors: more states than the kernel holds");
  const size_t lds = ((size_t)4 * (size_t)a.max_chunks + 2) * sizeof(double);  // <= 32 KB + 16
  return timed_launch(K_POSTERIORS, stream, err, [&] {
    for_dtype(a.dtype, [&](auto dt) {
      for_threads(a.max_chunks, [&](auto nt) {
        constexpr int NT = decltype(nt)::value, DT = decltype(dt)::value;
        hipLaunchKernelGGL((ctc_posteriors<NT, DT>), dim3((unsigned)a.n_utts), dim3(NT), lds, stream, a);
      });
    });
  });
}

// the row's threads and what they keep by the vocabulary alone: 16 lanes up to 64 labels, a wave up to 256 (four entries
// each), the workgroup above (four entries each up to 1024 labels, else sixteen; beyond 4096 labels the rest is formed twice)
int launch_ctc_grad_rows_on(const GradRowsArgs& a, hipStream_t stream, std::string* err) {
  if (a.n_utts <= 0 || a.n_rows <= 0) return 0;
  if (a.dtype < 0 || a.dtype > 3 || a.grad_dtype != (a.dtype == 1 ? 1 : 0) || a.n_labels < 1 || a.n_rows > (int64_t)0x7FFFFFFF)
    return bad_launch(err, "ctc_grad_rows: bad arguments");
  const int V = a.n_labels;
  const int rpb = V <= 64 ? 16 : V <= 256 ? 4 : 1;
  const dim3 grid((unsigned)((a.n_rows + rpb - 1) / rpb)), block(ALIGN_THREADS);
  return timed_launch(K_GRAD_ROWS, stream, err, [&] {
    for_dtype(a.dtype, [&](auto dt) {
      constexpr int DT = decltype(dt)::value;
      typedef typename std::conditional<DT == 1, double, float>::type GT;
      if (V <= 64) hipLaunchKernelGGL((ctc_grad_rows<16, 4, DT, GT>), grid, block, 0, stream, a);
      else if (V <= 256) hipLaunchKernelGGL((ctc_grad_rows<64, 4, DT, GT>), grid, block, 0, stream, a);
      else if (V <= 1024) hipLaunchKernelGGL((ctc_grad_rows<ALIGN_THREADS, 4, DT, GT>), grid, block, 0, stream, a);
      else hipLaunchKernelGGL((ctc_grad_rows<ALIGN_THREADS, 16, DT, GT>), grid, block, 0, stream, a);
    });
  });
}

int launch_ctc_find_on(const FindArgs& a, int wave, hipStream_t stream, std::string* err) {
  if (a.n_phrases <= 0) return 0;
  if (a.dtype < 0 || a.dtype > 3 || a.max_hits < 1 || a.max_hits > FIND_MAX_HITS || a.max_chunks < 1 ||
      a.max_chunks > (wave ? find_chunks(FIND_WAVE_MAX_LABELS) : find_chunks(ALIGN_MAX_LABELS)))
    return bad_launch(err, "ctc_find: more states or hits than the kernel holds");
  const size_t lds = (size_t)2 * (size_t)a.max_chunks * (sizeof(double) + sizeof(int32_t));  // (ctc_find) <= 24 KB
  return timed_launch(K_FIND, stream, err, [&] {
    for_dtype(a.dtype, [&](auto dt) {
      constexpr int DT = decltype(dt)::value;
      if (wave) {
        hipLaunchKernelGGL(ctc_find_wave<DT>, dim3((unsigned)((a.n_phrases + FORWARD_WAVES - 1) / FORWARD_WAVES)), dim3(ALIGN_THREADS), 0, stream, a);
        return;
      }
      for_threads(a.max_chunks, [&](auto nt) {
        constexpr int NT = decltype(nt)::value;
        hipLaunchKernelGGL((ctc_find<NT, DT>), dim3((unsigned)a.n_phrases), dim3(NT), lds, stream, a);
      });
    });
  });
}

}  // namespace be
}  // namespace ctc
