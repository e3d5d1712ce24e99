// ctc_align_hip.hip -- forced alignment and transcript likelihood on gfx950 (ctc_align.h): row_lse, the fp64 log-sum-exp of
// every frame row; ctc_viterbi, one workgroup per utterance over the blank / label / blank / ... states; ctc_forward and
// ctc_forward_wave, the sum over all alignments of a hypothesis, one workgroup / one wavefront each; ctc_posteriors, the
// forward-backward of an utterance's transcript, one workgroup each; ctc_grad_rows, the gradient of the likelihood from the
// posteriors a dense ctc_posteriors launch left, row by row; ctc_find and ctc_find_wave, the occurrences of a phrase inside
// an utterance, one workgroup / one wavefront each; row_lse_max and ctc_viterbi_gaps, the alignment of a target with gaps, one
// workgroup per utterance with its states in registers. A translation unit of its own.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "backend.h"
#include "ctc_align.h"

namespace ctc {
namespace be {

#define HIP_TRY_A(expr)                                                                  \
  do {                                                                                   \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess) {                                                              \
      if (err) *err = std::string(#expr) + ": " + hipGetErrorString(e_);                 \
      return -1;                                                                         \
    }                                                                                    \
  } while (0)

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

template <int G, int DT>
__global__ __launch_bounds__(256) void row_lse(RowLseArgs a) {
  constexpr int RPB = 256 / G;                            // rows per workgroup
  constexpr int ESZ = DT == 0 ? 4 : DT == 1 ? 8 : 2;      // bytes per element
  constexpr int EPV = 16 / ESZ;                           // elements per 16-byte vector
  constexpr int VPB = ALIGN_LSE_BLOCK / EPV;              // vectors per block of values
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
  // Which values a lane folds, and in which order, depends on the element index alone -- never on where the row lies in memory:
  // the same row gives the same bits whether it comes alone, inside a batch or out of a staging buffer.
  const bool vec = ((uintptr_t)p & 15u) == 0;
  const int nvec = V / EPV, tail = nvec * EPV;
  LseAcc acc = lse_empty();
  for (int i = tail + l; i < V; i += G) lse_push(acc, align_load(p, DT, (size_t)i));
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
    lse_push_block(acc, v);
  }
  CTC_UNROLL
  for (int off = G / 2; off >= 1; off >>= 1) {
    LseAcc o;
    o.m = __shfl_xor(acc.m, off, G);
    o.s = __shfl_xor(acc.s, off, G);
    acc = lse_merge(acc, o);
  }
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
// with: a second 8 bytes per row, no new arithmetic. The same lanes fold the same values in the same order and the same
// butterfly merges them, so the log-sum-exp has row_lse's bits, wherever the row lies in memory. The rows of a probability-
// like utterance, which row_lse skips, take the same loads and a plain maximum, without an exponential. Every logit is
// still read once.
// ---------------------------------------------------------------------------------------------
template <int G, int DT, bool MAX_ONLY>
__device__ __forceinline__ LseAcc row_fold(const char* p, int V, int l) {
  constexpr int ESZ = DT == 0 ? 4 : DT == 1 ? 8 : 2;      // bytes per element
  constexpr int EPV = 16 / ESZ;                           // elements per 16-byte vector
  constexpr int VPB = ALIGN_LSE_BLOCK / EPV;              // vectors per block of values
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

// kernel times: one pair of events per launch since the last reset
struct EventLog {
  std::vector<hipEvent_t> ev;
  size_t used = 0;
  int next(hipEvent_t* out, std::string* err) {
    if (used == ev.size()) {
      hipEvent_t e;
      HIP_TRY_A(hipEventCreate(&e));
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
static EventLog g_lse_log, g_vit_log, g_fwd_log, g_post_log, g_grad_log, g_find_log, g_lsemax_log, g_vitgaps_log;

void align_timing_reset() {
  g_lse_log.used = g_vit_log.used = g_fwd_log.used = g_post_log.used = g_grad_log.used = g_find_log.used = 0;
  g_lsemax_log.used = g_vitgaps_log.used = 0;
}
void align_gaps_timing(double* row_lse_max_ms, double* viterbi_gaps_ms) {
  *row_lse_max_ms = g_lsemax_log.total();
  *viterbi_gaps_ms = g_vitgaps_log.total();
}
double forward_timing() { return g_fwd_log.total(); }
double posteriors_timing() { return g_post_log.total(); }
double grad_rows_timing() { return g_grad_log.total(); }
double find_timing() { return g_find_log.total(); }
void align_timing(double* row_lse_ms, double* viterbi_ms) {
  *row_lse_ms = g_lse_log.total();
  *viterbi_ms = g_vit_log.total();
}

template <int G>
static void launch_row_lse_g(const RowLseArgs& a, hipStream_t stream) {
  const dim3 grid((unsigned)((a.n_rows + (256 / G) - 1) / (256 / G))), block(256);
  if (a.dtype == 0) hipLaunchKernelGGL((row_lse<G, 0>), grid, block, 0, stream, a);
  else if (a.dtype == 1) hipLaunchKernelGGL((row_lse<G, 1>), grid, block, 0, stream, a);
  else if (a.dtype == 2) hipLaunchKernelGGL((row_lse<G, 2>), grid, block, 0, stream, a);
  else hipLaunchKernelGGL((row_lse<G, 3>), grid, block, 0, stream, a);
}

int launch_row_lse_on(const RowLseArgs& a, hipStream_t stream, std::string* err) {
  if (a.n_rows <= 0 || a.n_utts <= 0) return 0;
  if (a.dtype < 0 || a.dtype > 3 || a.n_labels < 1 || a.n_rows > (int64_t)0x7FFFFFFF * 4) {
    if (err) *err = "row_lse: bad arguments";
    return -1;
  }
  hipEvent_t e0, e1;
  if (g_lse_log.next(&e0, err) || g_lse_log.next(&e1, err)) return -1;
  HIP_TRY_A(hipEventRecord(e0, stream));
  if (a.n_labels >= 256) launch_row_lse_g<64>(a, stream);
  else if (a.n_labels >= 32) launch_row_lse_g<16>(a, stream);
  else launch_row_lse_g<4>(a, stream);
  HIP_TRY_A(hipGetLastError());
  HIP_TRY_A(hipEventRecord(e1, stream));
  return 0;
}

int launch_ctc_viterbi_on(const ViterbiArgs& a, hipStream_t stream, std::string* err) {
  if (a.n_utts <= 0) return 0;
  if (a.max_chunks < 1 || a.max_chunks > align_chunks(ALIGN_MAX_LABELS)) {
    if (err) *err = "ctc_viterbi: more states than two score columns in LDS hold";
    return -1;
  }
  const size_t lds = (size_t)2 * 4 * (size_t)a.max_chunks * sizeof(double);  // <= 64 KB
  hipEvent_t e0, e1;
  if (g_vit_log.next(&e0, err) || g_vit_log.next(&e1, err)) return -1;
  HIP_TRY_A(hipEventRecord(e0, stream));
  hipLaunchKernelGGL(ctc_viterbi, dim3((unsigned)a.n_utts), dim3(ALIGN_THREADS), lds, stream, a);
  HIP_TRY_A(hipGetLastError());
  HIP_TRY_A(hipEventRecord(e1, stream));
  return 0;
}

template <int G>
static void launch_row_lse_max_g(const RowLseArgs& a, double* rmax, hipStream_t stream) {
  const dim3 grid((unsigned)((a.n_rows + (256 / G) - 1) / (256 / G))), block(256);
  if (a.dtype == 0) hipLaunchKernelGGL((row_lse_max<G, 0>), grid, block, 0, stream, a, rmax);
  else if (a.dtype == 1) hipLaunchKernelGGL((row_lse_max<G, 1>), grid, block, 0, stream, a, rmax);
  else if (a.dtype == 2) hipLaunchKernelGGL((row_lse_max<G, 2>), grid, block, 0, stream, a, rmax);
  else hipLaunchKernelGGL((row_lse_max<G, 3>), grid, block, 0, stream, a, rmax);
}

// (the lanes per row by the vocabulary alone, as launch_row_lse_on picks them: the same grouping, the same bits)
int launch_row_lse_max_on(const RowLseArgs& a, double* rmax, hipStream_t stream, std::string* err) {
  if (a.n_rows <= 0 || a.n_utts <= 0) return 0;
  if (a.dtype < 0 || a.dtype > 3 || a.n_labels < 1 || a.n_rows > (int64_t)0x7FFFFFFF * 4 || !rmax) {
    if (err) *err = "row_lse_max: bad arguments";
    return -1;
  }
  hipEvent_t e0, e1;
  if (g_lsemax_log.next(&e0, err) || g_lsemax_log.next(&e1, err)) return -1;
  HIP_TRY_A(hipEventRecord(e0, stream));
  if (a.n_labels >= 256) launch_row_lse_max_g<64>(a, rmax, stream);
  else if (a.n_labels >= 32) launch_row_lse_max_g<16>(a, rmax, stream);
  else launch_row_lse_max_g<4>(a, rmax, stream);
  HIP_TRY_A(hipGetLastError());
  HIP_TRY_A(hipEventRecord(e1, stream));
  return 0;
}

template <int DT>
static void launch_viterbi_gaps_dt(const ViterbiGapsArgs& a, hipStream_t stream) {
  const size_t lds = (size_t)2 * (size_t)a.max_chunks * sizeof(double);  // <= 16 KB
  if (a.max_chunks <= ALIGN_THREADS) hipLaunchKernelGGL((ctc_viterbi_gaps<ALIGN_THREADS, DT>), dim3((unsigned)a.n_utts), dim3(ALIGN_THREADS), lds, stream, a);
  else hipLaunchKernelGGL((ctc_viterbi_gaps<FORWARD_THREADS_MAX, DT>), dim3((unsigned)a.n_utts), dim3(FORWARD_THREADS_MAX), lds, stream, a);
}

int launch_ctc_viterbi_gaps_on(const ViterbiGapsArgs& a, hipStream_t stream, std::string* err) {
  if (a.n_utts <= 0) return 0;
  if (a.dtype < 0 || a.dtype > 3 || a.max_chunks < 1 || a.max_chunks > align_chunks(ALIGN_MAX_LABELS)) {
    if (err) *err = "ctc_viterbi_gaps: more states than the kernel holds";
    return -1;
  }
  hipEvent_t e0, e1;
  if (g_vitgaps_log.next(&e0, err) || g_vitgaps_log.next(&e1, err)) return -1;
  HIP_TRY_A(hipEventRecord(e0, stream));
  if (a.dtype == 0) launch_viterbi_gaps_dt<0>(a, stream);
  else if (a.dtype == 1) launch_viterbi_gaps_dt<1>(a, stream);
  else if (a.dtype == 2) launch_viterbi_gaps_dt<2>(a, stream);
  else launch_viterbi_gaps_dt<3>(a, stream);
  HIP_TRY_A(hipGetLastError());
  HIP_TRY_A(hipEventRecord(e1, stream));
  return 0;
}

template <int DT>
static void launch_forward_dt(const ForwardArgs& a, int wave, hipStream_t stream) {
  if (wave) {
    hipLaunchKernelGGL(ctc_forward_wave<DT>, dim3((unsigned)((a.n_hyps + FORWARD_WAVES - 1) / FORWARD_WAVES)), dim3(ALIGN_THREADS), 0, stream, a);
    return;
  }
  const size_t lds = (size_t)2 * (size_t)a.max_chunks * sizeof(double);  // <= 16 KB
  if (a.max_chunks <= ALIGN_THREADS) hipLaunchKernelGGL((ctc_forward<ALIGN_THREADS, DT>), dim3((unsigned)a.n_hyps), dim3(ALIGN_THREADS), lds, stream, a);
  else hipLaunchKernelGGL((ctc_forward<FORWARD_THREADS_MAX, DT>), dim3((unsigned)a.n_hyps), dim3(FORWARD_THREADS_MAX), lds, stream, a);
}

int launch_ctc_forward_on(const ForwardArgs& a, int wave, hipStream_t stream, std::string* err) {
  if (a.n_hyps <= 0) return 0;
  if (a.dtype < 0 || a.dtype > 3 || a.max_chunks < 1 || a.max_chunks > (wave ? align_chunks(FORWARD_WAVE_MAX_LABELS) : align_chunks(ALIGN_MAX_LABELS))) {
    if (err) *err = "ctc_forward: more states than the kernel holds";
    return -1;
  }
  hipEvent_t e0, e1;
  if (g_fwd_log.next(&e0, err) || g_fwd_log.next(&e1, err)) return -1;
  HIP_TRY_A(hipEventRecord(e0, stream));
  if (a.dtype == 0) launch_forward_dt<0>(a, wave, stream);
  else if (a.dtype == 1) launch_forward_dt<1>(a, wave, stream);
  else if (a.dtype == 2) launch_forward_dt<2>(a, wave, stream);
  else launch_forward_dt<3>(a, wave, stream);
  HIP_TRY_A(hipGetLastError());
  HIP_TRY_A(hipEventRecord(e1, stream));
  return 0;
}

template <int DT>
static void launch_posteriors_dt(const PosteriorsArgs& a, hipStream_t stream) {
  const size_t lds = ((size_t)4 * (size_t)a.max_chunks + 2) * sizeof(double);  // <= 32 KB + 16
  if (a.max_chunks <= ALIGN_THREADS) hipLaunchKernelGGL((ctc_posteriors<ALIGN_THREADS, DT>), dim3((unsigned)a.n_utts), dim3(ALIGN_THREADS), lds, stream, a);
  else hipLaunchKernelGGL((ctc_posteriors<FORWARD_THREADS_MAX, DT>), dim3((unsigned)a.n_utts), dim3(FORWARD_THREADS_MAX), lds, stream, a);
}

int launch_ctc_posteriors_on(const PosteriorsArgs& a, hipStream_t stream, std::string* err) {
  if (a.n_utts <= 0) return 0;
  if (a.dtype < 0 || a.dtype > 3 || a.max_chunks < 1 || a.max_chunks > align_chunks(ALIGN_MAX_LABELS)) {
    if (err) *err = "ctc_posteriors: more states than the kernel holds";
    return -1;
  }
  hipEvent_t e0, e1;
  if (g_post_log.next(&e0, err) || g_post_log.next(&e1, err)) return -1;
  HIP_TRY_A(hipEventRecord(e0, stream));
  if (a.dtype == 0) launch_posteriors_dt<0>(a, stream);
  else if (a.dtype == 1) launch_posteriors_dt<1>(a, stream);
  else if (a.dtype == 2) launch_posteriors_dt<2>(a, stream);
  else launch_posteriors_dt<3>(a, stream);
  HIP_TRY_A(hipGetLastError());
  HIP_TRY_A(hipEventRecord(e1, stream));
  return 0;
}

// the row's threads and what they keep by the vocabulary alone: 16 lanes up to 64 labels, a wave up to 256 (four entries
// each), the workgroup above (four entries each up to 1024 labels, else sixteen; beyond 4096 labels the rest is formed twice)
template <int DT, class GT>
static void launch_grad_rows_dt(const GradRowsArgs& a, hipStream_t stream) {
  const int V = a.n_labels;
  const int rpb = V <= 64 ? 16 : V <= 256 ? 4 : 1;
  const dim3 grid((unsigned)((a.n_rows + rpb - 1) / rpb)), block(ALIGN_THREADS);
  if (V <= 64) hipLaunchKernelGGL((ctc_grad_rows<16, 4, DT, GT>), grid, block, 0, stream, a);
  else if (V <= 256) hipLaunchKernelGGL((ctc_grad_rows<64, 4, DT, GT>), grid, block, 0, stream, a);
  else if (V <= 1024) hipLaunchKernelGGL((ctc_grad_rows<ALIGN_THREADS, 4, DT, GT>), grid, block, 0, stream, a);
  else hipLaunchKernelGGL((ctc_grad_rows<ALIGN_THREADS, 16, DT, GT>), grid, block, 0, stream, a);
}

int launch_ctc_grad_rows_on(const GradRowsArgs& a, hipStream_t stream, std::string* err) {
  if (a.n_utts <= 0 || a.n_rows <= 0) return 0;
  if (a.dtype < 0 || a.dtype > 3 || a.grad_dtype != (a.dtype == 1 ? 1 : 0) || a.n_labels < 1 || a.n_rows > (int64_t)0x7FFFFFFF) {
    if (err) *err = "ctc_grad_rows: bad arguments";
    return -1;
  }
  hipEvent_t e0, e1;
  if (g_grad_log.next(&e0, err) || g_grad_log.next(&e1, err)) return -1;
  HIP_TRY_A(hipEventRecord(e0, stream));
  if (a.dtype == 0) launch_grad_rows_dt<0, float>(a, stream);
  else if (a.dtype == 1) launch_grad_rows_dt<1, double>(a, stream);
  else if (a.dtype == 2) launch_grad_rows_dt<2, float>(a, stream);
  else launch_grad_rows_dt<3, float>(a, stream);
  HIP_TRY_A(hipGetLastError());
  HIP_TRY_A(hipEventRecord(e1, stream));
  return 0;
}

template <int DT>
static void launch_find_dt(const FindArgs& a, int wave, hipStream_t stream) {
  if (wave) {
    hipLaunchKernelGGL(ctc_find_wave<DT>, dim3((unsigned)((a.n_phrases + FORWARD_WAVES - 1) / FORWARD_WAVES)), dim3(ALIGN_THREADS), 0, stream, a);
    return;
  }
  const size_t lds = (size_t)2 * (size_t)a.max_chunks * (sizeof(double) + sizeof(int32_t));  // <= 24 KB
  if (a.max_chunks <= ALIGN_THREADS) hipLaunchKernelGGL((ctc_find<ALIGN_THREADS, DT>), dim3((unsigned)a.n_phrases), dim3(ALIGN_THREADS), lds, stream, a);
  else hipLaunchKernelGGL((ctc_find<FORWARD_THREADS_MAX, DT>), dim3((unsigned)a.n_phrases), dim3(FORWARD_THREADS_MAX), lds, stream, a);
}

int launch_ctc_find_on(const FindArgs& a, int wave, hipStream_t stream, std::string* err) {
  if (a.n_phrases <= 0) return 0;
  if (a.dtype < 0 || a.dtype > 3 || a.max_hits < 1 || a.max_hits > FIND_MAX_HITS || a.max_chunks < 1 ||
      a.max_chunks > (wave ? find_chunks(FIND_WAVE_MAX_LABELS) : find_chunks(ALIGN_MAX_LABELS))) {
    if (err) *err = "ctc_find: more states or hits than the kernel holds";
    return -1;
  }
  hipEvent_t e0, e1;
  if (g_find_log.next(&e0, err) || g_find_log.next(&e1, err)) return -1;
  HIP_TRY_A(hipEventRecord(e0, stream));
  if (a.dtype == 0) launch_find_dt<0>(a, wave, stream);
  else if (a.dtype == 1) launch_find_dt<1>(a, wave, stream);
  else if (a.dtype == 2) launch_find_dt<2>(a, wave, stream);
  else launch_find_dt<3>(a, wave, stream);
  HIP_TRY_A(hipGetLastError());
  HIP_TRY_A(hipEventRecord(e1, stream));
  return 0;
}

}  // namespace be
}  // namespace ctc
