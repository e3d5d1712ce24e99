// backend_hip.hip -- the product backend: HIP kernels for gfx950 (MI355X, CDNA4, wave64).
//
// It owns the decode stream, the copy stream and the stage timing events, and fronts every launcher of backend.h on them. The
// large stages are translation units of their own -- frame_prune_hip.hip (frame prune and input sniff), beam_wave_hip.hip and
// beam_group_hip.hip (the two beam kernels), ctc_align_hip.hip (the transcript kernels); what is left here, top to bottom:
//
//   init, bind_thread, alloc*, h2d*, d2h*, d2d, zero, sync     device, streams, memory, copies
//   last_timing, last_prune_ms                                 prune and beam stage times from g_ev[0..2]
//   launch_prune, launch_sniff_exact                           fronts of frame_prune_hip.hip: they record g_ev[0] / g_ev[1]
//   assemble_texts                                             decode_batch's texts on the device (text_wave.h), a wave per utterance
//   utt_weigh, utt_place                                       the wave kernel's launch order and per-utterance weights
//   wave_kernel_chosen, hot_tok_build, launch_beam             which beam kernel; per-utterance hot words; the beam launch, g_ev[2]
//   token_logp, launch_token_logp                              token confidences from the survivor arrays (token_logp.h)
//   launch_ctc_* / launch_row_lse*                             fronts of ctc_align_hip.hip
//   surv_ledger_append, token_logp_ledger, launch_ledger_*     the streaming survivor ledger (surv_ledger.h)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <vector>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "backend.h"
#include "beam_core.h"
#include "beam_wave.h"
#include "hip_try.h"
#include "text_wave.h"
#include "wave_ops_hip.h"

namespace ctc {
namespace be {

// Every backend call acts on the decode stream, except h2d_2d_overlapped: its copies run on a stream of their own, under the
// kernels queued on the decode stream (api.cpp: decode_host_sliced). Calls are serialised by the caller's device mutex.
static hipStream_t g_stream = nullptr;       // the decode stream
static hipStream_t g_copy_stream = nullptr;  // h2d_2d_overlapped
static hipEvent_t g_ev[3] = {nullptr, nullptr, nullptr};
static int g_device = -1;
static int g_cus = 256;  // compute units of the device (MI355X: 256)
static bool g_timing_valid = false;

const char* name() { return "hip-gfx950"; }

// One process drives ONE GPU (the multi-GPU layout is one process per GPU): the stream, the
// timing events and every workspace belong to the device of the first decoder. A later decoder asking for a
// different device is refused instead of silently mixing that device's kernels with this device's stream.
int init(int device, std::string* err) {
  if (g_stream) {
    int n = 0;
    (void)hipGetDeviceCount(&n);
    if (device < 0 || device >= n) device = 0;
    if (device != g_device) {
      if (err) *err = "this process already decodes on device " + std::to_string(g_device) + "; device " + std::to_string(device) +
                      " needs its own process (one process per GPU)";
      return -1;
    }
    return bind_thread(err);
  }
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0) {
    if (err) *err = "no HIP device available (libctcdec has no CPU fallback)";
    return -1;
  }
  if (device < 0 || device >= n) device = 0;
  HIP_TRY(hipSetDevice(device));
  if (!g_stream) {
    HIP_TRY(hipStreamCreateWithFlags(&g_stream, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&g_copy_stream, hipStreamNonBlocking));
    for (int k = 0; k < 3; ++k) HIP_TRY(hipEventCreate(&g_ev[k]));
  }
  g_device = device;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) g_cus = prop.multiProcessorCount;
  return 0;
}

// Host threads other than the one that created the decoder start with device 0 current: every entry point that
// allocates, copies or launches binds the calling thread to the decoder's device first.
int bind_thread(std::string* err) {
  if (g_device >= 0) HIP_TRY(hipSetDevice(g_device));
  return 0;
}
int current_device() { return g_device; }

void* alloc(size_t bytes, std::string* err) {
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, bytes ? bytes : 16);
  if (e != hipSuccess) {
    if (err) *err = std::string("hipMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e);
    return nullptr;
  }
  return p;
}
void release(void* p) { (void)hipFree(p); }
void* alloc_host(size_t bytes, std::string* err) {
  void* p = nullptr;
  hipError_t e = hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocDefault);
  if (e != hipSuccess) {
    if (err) *err = std::string("hipHostMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e);
    return nullptr;
  }
  return p;
}
void release_host(void* p) { (void)hipHostFree(p); }
int h2d(void* d, const void* s, size_t n, std::string* err) {
  HIP_TRY(hipMemcpyAsync(d, s, n, hipMemcpyHostToDevice, g_stream));
  HIP_TRY(hipStreamSynchronize(g_stream));  // the source is caller memory that may be reused
  return 0;
}
int h2d_2d_overlapped(void* d, size_t dpitch, const void* s, size_t spitch, size_t width, size_t height, std::string* err) {
  hipStream_t copy = g_copy_stream;
  if (height == 0 || width == 0) return 0;
  if (height == 1 || (dpitch == width && spitch == width)) HIP_TRY(hipMemcpyAsync(d, s, width * height, hipMemcpyHostToDevice, copy));
  else HIP_TRY(hipMemcpy2DAsync(d, dpitch, s, spitch, width, height, hipMemcpyHostToDevice, copy));
  HIP_TRY(hipStreamSynchronize(copy));
  return 0;
}
int d2h(void* d, const void* s, size_t n, std::string* err) {
  HIP_TRY(hipMemcpyAsync(d, s, n, hipMemcpyDeviceToHost, g_stream));
  HIP_TRY(hipStreamSynchronize(g_stream));
  return 0;
}
int d2d(void* d, const void* s, size_t n, std::string* err) {
  HIP_TRY(hipMemcpyAsync(d, s, n, hipMemcpyDeviceToDevice, g_stream));
  return 0;
}
int zero(void* d, size_t n, std::string* err) {
  HIP_TRY(hipMemsetAsync(d, 0, n, g_stream));
  return 0;
}
int sync(std::string* err) {
  HIP_TRY(hipStreamSynchronize(g_stream));
  return 0;
}

int d2h_async(void* d, const void* s, size_t n, std::string* err) {
  HIP_TRY(hipMemcpyAsync(d, s, n, hipMemcpyDeviceToHost, g_stream));
  return 0;
}
int h2d_async(void* d, const void* s, size_t n, std::string* err) {
  HIP_TRY(hipMemcpyAsync(d, s, n, hipMemcpyHostToDevice, g_stream));
  return 0;
}
int cus() { return g_cus; }

void last_timing(double* prune_ms, double* beam_ms) {
  *prune_ms = 0;
  *beam_ms = 0;
  if (!g_timing_valid) return;
  float a = 0, b = 0;
  if (hipEventSynchronize(g_ev[2]) != hipSuccess) return;
  if (hipEventElapsedTime(&a, g_ev[0], g_ev[1]) == hipSuccess) *prune_ms = a;
  if (hipEventElapsedTime(&b, g_ev[1], g_ev[2]) == hipSuccess) *beam_ms = b;
}

double last_prune_ms() {
  float ms = 0.f;
  if (!g_ev[1] || hipEventSynchronize(g_ev[1]) != hipSuccess) return 0.0;
  return hipEventElapsedTime(&ms, g_ev[0], g_ev[1]) == hipSuccess ? (double)ms : 0.0;
}

// Frame prune: the kernels and the choice among them live in frame_prune_hip.hip; the decode stream and the stage's two timing
// events are this file's.
int launch_prune_on(const PruneArgs& a, hipStream_t stream, std::string* err);
int launch_sniff_exact_on(const PruneArgs& a, hipStream_t stream, std::string* err);
int launch_prune(const PruneArgs& a, std::string* err) {
  if (a.pass == 0) {
    g_timing_valid = false;
    HIP_TRY(hipEventRecord(g_ev[0], g_stream));
  }
  if (launch_prune_on(a, g_stream, err)) return -1;
  HIP_TRY(hipEventRecord(g_ev[1], g_stream));
  return 0;
}
int launch_sniff_exact(const PruneArgs& a, std::string* err) { return launch_sniff_exact_on(a, g_stream, err); }

// workgroup kernel: one workgroup per utterance (beam_core.h), compiled in its own translation unit (beam_group_hip.hip).
// kind: 0 = four waves per utterance, 1 = eight, 2 = several language models (four waves)
int launch_group(const BeamArgs& a, const LdsShape& shape, size_t lds, int kind, hipStream_t stream, std::string* err);
// wave kernel: one wavefront per utterance (beam_wave.h), compiled in its own translation unit (beam_wave_hip.hip)
int launch_wave(const BeamArgs& a, hipStream_t stream, std::string* err);

// decode_batch (params.texts_only): the best beam's text of every utterance, assembled on the device. One wave per
// utterance walks the emission chain leaf to root through LDS windows and writes the UTF-8 bytes into the utterance's
// scratch area (text_wave.h), then copies them to a block of the text pool. A launch of its own, behind the beam kernel:
// all the chain walks run side by side instead of one at the tail of every beam wave.
struct TextGpuCtx {
  int lane;
  __device__ __forceinline__ void wsync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  __device__ __forceinline__ uint64_t ballot(bool p) { return __ballot(p); }
  __device__ __forceinline__ int clz64(uint64_t x) { return __clzll((long long)x); }
  __device__ __forceinline__ uint32_t wave_excl_sum_u32(uint32_t v) {
    uint32_t incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t o = (uint32_t)__shfl_up((int)incl, off, 64);
      if (lane >= off) incl += o;
    }
    return incl - v;
  }
  __device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
    int x = (int)v;
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false);
    return (uint32_t)__builtin_amdgcn_readlane(x, 63);
  }
};

__global__ __launch_bounds__(64) void assemble_texts(BeamArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[TEXT_LDS_BYTES];
  const int u = blockIdx.x;
  const int lane = threadIdx.x;
  if (a.n_out[u] == 0) return;
  OutBeam& ob = a.out[(size_t)u * a.out_stride];
  uint8_t* scratch = a.text_scratch + a.text_soff[u];
  const uint32_t cap = (uint32_t)(a.text_soff[u + 1] - a.text_soff[u]);
  TextLds L;
  text_lds_carve(L, (CTC_LDS char*)smem);
  TextGpuCtx ctx{lane};
  const uint32_t pos = wave_text_backwards(ctx, L, a.emit_nodes + a.emit_off[u], a.tables, ob.pad[1], scratch, cap,
                                           (uint32_t)(a.emit_off[u + 1] - a.emit_off[u]));
  uint32_t len = cap - pos;
  unsigned long long base = 0;
  if (lane == 0) {
    base = atomicAdd(a.tok_pool_head + 1, (unsigned long long)len);
    if (base + len > a.text_pool_cap) {
      a.status[u] |= ST_TOK_OVERFLOW;
      base = 0;
      len = 0;
    }
    ob.tok_off = (uint32_t)base;
    ob.tok_cnt = len;
    ob.pad[0] = (uint32_t)(base >> 32);
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");  // (every lane reads bytes other lanes wrote)
  __builtin_amdgcn_wave_barrier();
  len = (uint32_t)__builtin_amdgcn_readfirstlane((int)len);
  const uint32_t blo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
  const uint32_t bhi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32));
  base = ((unsigned long long)bhi << 32) | blo;
  for (uint32_t k = (uint32_t)lane; k < len; k += 64u) a.text_pool[base + k] = scratch[pos + k];
}

// ---- what a frame of each utterance will cost, before the wave kernel decodes it (round 6) -------------------------------------
// The wave kernel's launch lasts as long as its slowest wave. What makes a wave slow is its utterance's candidates per frame
// (live beams x surviving labels: r = 0.97 with a wave's natural lifetime, profiles/r06_weigh_predictors.txt). The live beams are
// known only once the utterance is decoded, but the surviving labels are what the prune stage has just counted, and they explain
// a fifth of it (r = 0.47) -- enough to let the launch know its probably-heavy utterances BEFORE it starts:
//   utt_weigh  (one wave per utterance): cost per frame = WEIGH_C0 + survivors per frame, and the utterance's total;
//   utt_place  (sixteen utterances per workgroup): ranks the totals by counting and deals the utterances out -- heaviest first: workgroup
//              b of a launch lands in slot b / 1024 of SIMD b mod 1024, so the first 1024 are the oldest waves of their SIMDs, and
//              age is the arbiter's tie-break -- in a snake over the SIMD count, so that each SIMD's four waves add up to about the
//              same predicted work; every workgroup is left the relative weight of its utterance (BeamArgs::block_weight), by which
//              WaveGpuCtx::frame_done scales the frames it still has to decode.
// Measured (profiles/r06_ab_weigh_place.log, r06_ab_weigh_gain_snake.log): the dispatch order is worth 1.0 ms of the 17-ms launch
// (lightest first: +1.3 ms), the snake 0.2 ms, the weights in the priority rule 0.1 ms.
// Which utterance a workgroup decodes never changes what it computes (tests/test_full_occupancy.py: placement test).
constexpr float WEIGH_C0 = 4.0f;
constexpr float WEIGH_GAIN = 4.0f;  // (the regression of a wave's natural lifetime on this weight has slope ~3: profiles/r06_weigh_*.txt)
constexpr int PLACE_MAX = 8192;  // utterances utt_place ranks (LDS: 4 bytes each); larger launches keep their order
struct WeighArgs {
  const int64_t* utt_row0;
  const uint32_t* surv_cnt;
  int32_t n_utts;
  float* total;        // [n_utts] WEIGH_C0 * frames + survivors
  float* per_frame;    // [n_utts]
  const int32_t* given_order;  // or nullptr: utt_place decides
  int32_t* order;      // [n_utts] out (given_order == nullptr)
  float* block_weight; // [n_utts] out
  int32_t simds;
  float gain;          // block_weight = 1 + gain * (relative cost per frame - 1)
  int32_t snake;       // odd generations dealt out in reverse
};
__global__ __launch_bounds__(64) void utt_weigh(WeighArgs a) {
  const int u = blockIdx.x;
  const int lane = threadIdx.x;
  const int64_t r0 = a.utt_row0[u], r1 = a.utt_row0[u + 1];
  double c = 0.0;
  {
    uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;  // (four loads in flight per trip)
    for (int64_t r = r0 + lane; r < r1; r += 256) {
      const uint32_t n0 = a.surv_cnt[r], n1 = r + 64 < r1 ? a.surv_cnt[r + 64] : 0u, n2 = r + 128 < r1 ? a.surv_cnt[r + 128] : 0u,
                     n3 = r + 192 < r1 ? a.surv_cnt[r + 192] : 0u;
      c0 += n0; c1 += n1; c2 += n2; c3 += n3;
    }
    c = (double)c0 + (double)c1 + (double)c2 + (double)c3;
  }
  c = wave_sum(c);
  if (lane == 0) {
    const float T = (float)(r1 - r0);
    const float tot = WEIGH_C0 * T + (float)c;
    const float pf = T > 0.f ? tot / T : WEIGH_C0;
    a.total[u] = tot;
    a.per_frame[u] = pf;  // (their sum is taken by utt_place's workgroups themselves: thousands of atomics on one address cost 40 us)
  }
}
// 16 utterances per workgroup of 256 threads: sixteen lanes share the count of one utterance's rank (a single workgroup ranking
// 4096 totals took 0.7 ms -- most of what the placement saved)
constexpr int PLACE_PER_BLOCK = 16;
__global__ __launch_bounds__(256) void utt_place(WeighArgs a) {
  __shared__ float w[PLACE_MAX];
  __shared__ float part_sum[4];
  const int n = a.n_utts;
  {  // the launch's mean cost per frame (every workgroup adds the per-utterance values up itself)
    float acc = 0.f;
    for (int v = threadIdx.x; v < n; v += blockDim.x) acc += a.per_frame[v];
    acc = (float)wave_sum((double)acc);
    if ((threadIdx.x & 63) == 0) part_sum[threadIdx.x >> 6] = acc;
    __syncthreads();
  }
  const float scale = (float)n / ((part_sum[0] + part_sum[1]) + (part_sum[2] + part_sum[3]));
  const int u = blockIdx.x * PLACE_PER_BLOCK + (threadIdx.x >> 4), part = threadIdx.x & 15;
  if (a.given_order || n > PLACE_MAX || a.simds < 0) {  // weights only
    if (part == 0 && u < n) {
      const int v = a.given_order ? a.given_order[u] : u;
      a.block_weight[u] = 1.f + a.gain * (a.per_frame[v] * scale - 1.f);
    }
    return;
  }
  for (int v = threadIdx.x; v < n; v += blockDim.x) w[v] = a.total[v];
  __syncthreads();
  const int uu = u < n ? u : 0;
  const float mine = w[uu];
  int rank = 0;
  for (int v = part; v < n; v += 16) {
    const float x = w[v];
    rank += (x > mine || (x == mine && v < uu)) ? 1 : 0;
  }
  rank += __shfl_xor(rank, 1, 64);
  rank += __shfl_xor(rank, 2, 64);
  rank += __shfl_xor(rank, 4, 64);
  rank += __shfl_xor(rank, 8, 64);
  if (part == 0 && u < n) {
    const int S = a.simds;
    const int g = rank / S, k = rank - g * S;
    const int len = n - g * S < S ? n - g * S : S;
    int b = g * S + (((g & 1) && a.snake == 1) ? len - 1 - k : k);
    if (a.snake == 2) b = n - 1 - rank;  // (diagnostics: lightest first)
    a.order[b] = u;
    a.block_weight[b] = 1.f + a.gain * (a.per_frame[u] * scale - 1.f);
  }
}

static int g_last_kernel = 0;  // 1: wave kernel, 2: workgroup kernel
int last_beam_kernel() { return g_last_kernel; }

bool beam_kernel_depends_on_input(const BeamArgs& a) {
  return !getenv("CTCDEC_BEAM_KERNEL") && a.n_utts > 0 && a.n_utts <= g_cus && wave_eligible(a.tables, a.params) &&
         a.max_import <= wave_bucket(a.params.beam_width);
}

bool wave_kernel_chosen(const BeamArgs& a) {
  const char* force = getenv("CTCDEC_BEAM_KERNEL");
  // Small batches (at most one utterance per CU): by the input. Round 5 measured one utterance per call on real-posterior-like
  // input (371 x 29, ~1.3 survivors a frame, most frames consumed as single-label runs): 1.01 ms on one wave against 1.69 ms
  // on the workgroup kernel; on the bench input (~6 survivors a frame) 11.3 against 10.5 ms for one utterance; on flat logits
  // (29 survivors a frame, thousands of candidates) the workgroup kernel is four times faster. Hence: the wave kernel below 3
  // survivors a frame; unknown (surv_x16 == 0: the caller did not ask) the workgroup kernel. Between one and two utterances
  // per CU the density says too little -- 512 bench utterances 11.5 vs 12.1 ms in favour of the wave kernel, 512 utterances of
  // BASELINE configs[2] (32 character labels, a 4-gram: ~5 survivors but many live beams) 31.7 vs 17.9 ms against it: the
  // workgroup kernel stays.
  bool small_group = true;
  if (a.surv_x16 > 0 && a.n_utts <= g_cus) small_group = a.surv_x16 > 3 * 16;
  const bool want_group = force ? force[0] == 'g' : (a.n_utts <= 2 * g_cus && small_group);
  // (streaming: a stream may carry in more beams than this call's beam_width -- up to the workgroup kernel's table)
  return a.n_utts > 0 && !want_group && wave_eligible(a.tables, a.params) && a.max_import <= wave_bucket(a.params.beam_width);
}

// Per-label hot-word view of every set of a call with per-utterance hot words (what HostHotwords::build does on the host for
// the call-wide set, host_tables.cpp): one wave per set, lanes over the labels. A label whose clean text is a prefix of one of
// the set's hot words gets {shortest such word, is itself a hot word}, every other label {0, 0}.
__global__ __launch_bounds__(64) void hot_tok_build(const HotSet* sets, int32_t n_sets, const TokInfo* tok, uint32_t n_labels) {
  const int32_t k = (int32_t)blockIdx.x;
  if (k >= n_sets) return;
  const HotSet hs = sets[k];
  TokHot* out = const_cast<TokHot*>(hs.tok_hot);
  for (uint32_t i = threadIdx.x; i < n_labels; i += 64) {
    const TokInfo& t = tok[i];
    uint32_t ml = 0, cp = 0;
    TokHot v{0u, 0u};
    if (t.len_clean > 0 && hot_lookup(hs.hot, hs.hot_mask, t.h_clean, &ml, &cp)) v = TokHot{ml, cp};
    out[i] = v;
  }
}

int launch_beam(const BeamArgs& a, std::string* err) {
  if (a.hot_sets && a.n_hot_sets > 0 && a.n_utts > 0) {
    hipLaunchKernelGGL(hot_tok_build, dim3((unsigned)a.n_hot_sets), dim3(64), 0, g_stream, a.hot_sets, a.n_hot_sets, a.tables.tok,
                       a.tables.n_labels);
    HIP_TRY(hipGetLastError());
  }
  // Two kernels for the same recursion. A lone utterance's frame takes about the same time in both (measured in round 4 on
  // the bench input: 11.3 us on the workgroup kernel's eight waves, 11.4 us on one wave), but a CU holds two workgroups
  // against sixteen waves and one wave needs an eighth of the issue slots per utterance: the wave kernel wins as soon as
  // there are more utterances than the workgroup kernel can hold at once (512 utterances: 12.6 ms either way;
  // 1024: 14.9 vs 24.4 ms; 4096: 19.3 ms). Dense frames are the exception: ~2 500 candidates a frame (BASELINE configs[1],
  // 256 utterances) take 38 ms on the workgroup kernel and 160 ms on one wave. CTCDEC_BEAM_KERNEL=wave|group overrides the
  // batch-size rule (tests, tuning; `wave` still falls back when the decode is not eligible for it).
  const bool wave = a.pay && wave_kernel_chosen(a);
  if (wave) {
    BeamArgs wa = a;
    // issue priority among the waves that share a SIMD (WaveGpuCtx::frame_done). CTCDEC_WAVE_PRIO=none | rot<k> | dyn
    // Default: by remaining work (measured on the 4096-utterance bench launch, round 6: 17.95 -> 17.1 ms; rot5 the same; the
    // waves of a launch end 12.3 .. 16.1 ms (5th .. 95th percentile) apart without it, 13.6 .. 15.2 ms with it; batches of one
    // wave per SIMD or fewer are unaffected).
    const char* pr = getenv("CTCDEC_WAVE_PRIO");
    // (round 6, second half) "weigh" = dyn with every remaining frame weighed by the utterance's survivors per frame, and the
    // heavy utterances dispatched first / dealt out evenly over the SIMDs (utt_weigh, utt_place): the default for launches of
    // more than one wave per SIMD
    wa.prio_mode = a.n_utts > 4 * g_cus ? 33 : 32;
    if (pr && pr[0] == 'n') wa.prio_mode = 0;
    if (pr && pr[0] == 'r') wa.prio_mode = 1 + (pr[1] && pr[2] && pr[3] ? atoi(pr + 3) & 15 : 5);
    if (pr && pr[0] == 'd') wa.prio_mode = 32;
    if (pr && pr[0] == 'w') wa.prio_mode = 33;
    wa.progress = nullptr;
    wa.total_frames = 0;
    wa.inv_n_utts = 0.f;
    wa.block_weight = nullptr;
    const bool dump_times = getenv("CTCDEC_WAVE_TIMES") != nullptr;
    if (wa.prio_mode >= 32 || dump_times) {
      static unsigned long long* g_progress = nullptr;
      if (!g_progress) HIP_TRY(hipMalloc((void**)&g_progress, 16));
      HIP_TRY(hipMemsetAsync(g_progress, 0, 16, g_stream));
      wa.progress = g_progress;
      wa.total_frames = (unsigned long long)a.total_rows;
      wa.inv_n_utts = 1.0f / (float)a.n_utts;
      if (a.total_rows >= (1ll << 32)) wa.prio_mode = 0;
      if (wa.prio_mode == 33 || dump_times) {  // (a dump carries the weights along)
        static float* g_weigh = nullptr;  // total | per_frame | block_weight | order
        static int g_weigh_cap = 0;
        if (a.n_utts > g_weigh_cap) {
          if (g_weigh) HIP_TRY(hipFree(g_weigh));
          g_weigh = nullptr;
          g_weigh_cap = 0;
          HIP_TRY(hipMalloc((void**)&g_weigh, (size_t)a.n_utts * 16));
          g_weigh_cap = a.n_utts;
        }
        WeighArgs w;
        w.utt_row0 = a.utt_row0;
        w.surv_cnt = a.surv_cnt;
        w.n_utts = a.n_utts;
        w.total = g_weigh;
        w.per_frame = g_weigh + (size_t)a.n_utts;
        w.block_weight = g_weigh + (size_t)a.n_utts * 2;
        w.order = (int32_t*)(g_weigh + (size_t)a.n_utts * 3);
        const bool keep_order = a.order != nullptr || getenv("CTCDEC_NO_PLACE") != nullptr || a.n_utts > PLACE_MAX || wa.prio_mode != 33;
        w.given_order = a.order;               // (a ragged multi-round launch keeps its longest-first order)
        w.simds = keep_order ? -1 : 4 * g_cus;  // -1: weights only
        w.gain = getenv("CTCDEC_WEIGH_GAIN") ? (float)atof(getenv("CTCDEC_WEIGH_GAIN")) : WEIGH_GAIN;
        w.snake = getenv("CTCDEC_PLACE_SNAKE") ? atoi(getenv("CTCDEC_PLACE_SNAKE")) : 1;
        hipLaunchKernelGGL(utt_weigh, dim3((unsigned)a.n_utts), dim3(64), 0, g_stream, w);
        hipLaunchKernelGGL(utt_place, dim3((unsigned)((a.n_utts + PLACE_PER_BLOCK - 1) / PLACE_PER_BLOCK)), dim3(256), 0, g_stream, w);
        HIP_TRY(hipGetLastError());
        wa.block_weight = w.block_weight;
        if (!keep_order) wa.order = w.order;
      }
    }
    // diagnostics: when and where each wave ran -> CTCDEC_WAVE_TIMES=<file> (n_utts x 4 uint64; synchronous)
    const char* wt = getenv("CTCDEC_WAVE_TIMES");
    wa.wave_clock = nullptr;
    if (wt && wt[0]) HIP_TRY(hipMalloc((void**)&wa.wave_clock, (size_t)a.n_utts * 32));
    const int rc = launch_wave(wa, g_stream, err);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    if (wa.wave_clock) {
      std::vector<unsigned long long> h((size_t)a.n_utts * 4);
      HIP_TRY(hipStreamSynchronize(g_stream));
      HIP_TRY(hipMemcpy(h.data(), wa.wave_clock, h.size() * 8, hipMemcpyDeviceToHost));
      HIP_TRY(hipFree(wa.wave_clock));
      if (FILE* f = fopen(wt, "wb")) {
        fwrite(h.data(), 8, h.size(), f);
        fclose(f);
      }
      if (wa.block_weight) {  // <file>.w: the relative weight of every workgroup's utterance (float32)
        std::vector<float> bw((size_t)a.n_utts);
        HIP_TRY(hipMemcpy(bw.data(), wa.block_weight, bw.size() * 4, hipMemcpyDeviceToHost));
        if (FILE* f = fopen((std::string(wt) + ".w").c_str(), "wb")) {
          fwrite(bw.data(), 4, bw.size(), f);
          fclose(f);
        }
      }
    }
    g_last_kernel = 1;
  } else if (a.n_utts > 0) {
    // Eight waves per utterance instead of four when every CU holds at most one utterance (the LDS of a workgroup allows
    // two per CU, the registers 2 x 256 threads or 1 x 512): measured on MI355X, 256 utterances x T=1000 -- BASELINE config 2
    // (~2 500 candidates per frame) 84.2 -> 70.4 ms in round 3, the headline workload (a few dozen candidates) 12.1 -> 11.8 ms.
    // That variant also takes its candidates in chunks of 1024 with a merge table of 4096 slots (it has the CU's LDS to
    // itself): config 2 in 38 ms (round 4). Otherwise four waves (512 utterances, beam 100: 256 threads 13.0 ms, 128 threads
    // 15.2 ms, 64 threads 19.7 ms for this kernel). CTCDEC_GROUP_THREADS=256|512 forces one.
    const char* gt = getenv("CTCDEC_GROUP_THREADS");
    const bool wide = a.tables.n_lms <= 1 && (gt ? gt[0] == '5' : a.n_utts <= g_cus);
    LdsShape shape = make_shape(a.params.beam_width, a.params.max_surv, group_cand(beam_bucket(a.params.beam_width), wide));
    size_t lds = lds_bytes(shape);
    if (lds > 160 * 1024) {
      if (err) *err = "beam table does not fit LDS (" + std::to_string(lds) + " bytes)";
      return -1;
    }
    int rc;
    rc = launch_group(a, shape, lds, a.tables.n_lms > 1 ? 2 : (wide ? 1 : 0), g_stream, err);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    g_last_kernel = 2;
  }
  if (a.n_utts > 0 && a.params.texts_only && a.text_scratch) {
    hipLaunchKernelGGL(assemble_texts, dim3((unsigned)a.n_utts), dim3(64), 0, g_stream, a);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(g_ev[2], g_stream));
  g_timing_valid = true;
  return 0;
}

// Token confidences: one token per lane. A token's frames are consecutive rows of the survivor arrays (mostly one or two; the
// lists hold a handful of labels), and the tokens of a beam come in frame order, so neighbouring lanes read neighbouring rows:
// scattered 2- and 8-byte reads that the L2 still holds from the beam stage. Nothing to share between lanes, no LDS.
template <int FOLD>
__global__ __launch_bounds__(256) void token_logp(TokenLogpArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_tokens) return;
  double v;
  const uint32_t missing = token_logp_of<FOLD>(a.runs[i], a.surv_cnt, a.surv_id, a.surv_lp, (uint32_t)a.max_surv, &v);
  a.out[i] = v;
  if (missing) atomicAdd(a.missing, missing);
}

static hipEvent_t g_logp_ev[2] = {nullptr, nullptr};
int launch_token_logp(const TokenLogpArgs& a, std::string* err) {
  if (a.n_tokens <= 0) return 0;
  if (!g_logp_ev[0])
    for (int k = 0; k < 2; ++k) HIP_TRY(hipEventCreate(&g_logp_ev[k]));
  const dim3 grid((unsigned)((a.n_tokens + 255) / 256)), block(256);
  HIP_TRY(hipEventRecord(g_logp_ev[0], g_stream));
  if (a.fold == LOGP_MEAN) hipLaunchKernelGGL(token_logp<LOGP_MEAN>, grid, block, 0, g_stream, a);
  else if (a.fold == LOGP_MIN) hipLaunchKernelGGL(token_logp<LOGP_MIN>, grid, block, 0, g_stream, a);
  else if (a.fold == LOGP_MAX) hipLaunchKernelGGL(token_logp<LOGP_MAX>, grid, block, 0, g_stream, a);
  else {
    if (err) *err = "unknown token_logp fold";
    return -1;
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(g_logp_ev[1], g_stream));
  return 0;
}
double last_token_logp_ms() {
  float ms = 0.f;
  if (!g_logp_ev[1] || hipEventSynchronize(g_logp_ev[1]) != hipSuccess) return 0.0;
  return hipEventElapsedTime(&ms, g_logp_ev[0], g_logp_ev[1]) == hipSuccess ? (double)ms : 0.0;
}

// Forced alignment: the kernels live in ctc_align_hip.hip and run on the decode stream like everything else
int launch_row_lse_on(const RowLseArgs& a, hipStream_t stream, std::string* err);
int launch_ctc_viterbi_on(const ViterbiArgs& a, hipStream_t stream, std::string* err);
int launch_ctc_forward_on(const ForwardArgs& a, int wave, hipStream_t stream, std::string* err);
int launch_ctc_forward(const ForwardArgs& a, int wave, std::string* err) { return launch_ctc_forward_on(a, wave, g_stream, err); }
int launch_ctc_posteriors_on(const PosteriorsArgs& a, hipStream_t stream, std::string* err);
int launch_ctc_posteriors(const PosteriorsArgs& a, std::string* err) { return launch_ctc_posteriors_on(a, g_stream, err); }
int launch_ctc_grad_rows_on(const GradRowsArgs& a, hipStream_t stream, std::string* err);
int launch_ctc_grad_rows(const GradRowsArgs& a, std::string* err) { return launch_ctc_grad_rows_on(a, g_stream, err); }
int launch_ctc_find_on(const FindArgs& a, int wave, hipStream_t stream, std::string* err);
int launch_ctc_find(const FindArgs& a, int wave, std::string* err) { return launch_ctc_find_on(a, wave, g_stream, err); }
int launch_row_lse(const RowLseArgs& a, std::string* err) { return launch_row_lse_on(a, g_stream, err); }
int launch_ctc_viterbi(const ViterbiArgs& a, std::string* err) { return launch_ctc_viterbi_on(a, g_stream, err); }
int launch_ctc_viterbi_long_on(const ViterbiLongArgs& a, hipStream_t stream, std::string* err);
int launch_ctc_viterbi_long(const ViterbiLongArgs& a, std::string* err) { return launch_ctc_viterbi_long_on(a, g_stream, err); }
int launch_row_lse_max_on(const RowLseArgs& a, double* rmax, hipStream_t stream, std::string* err);
int launch_row_lse_max(const RowLseArgs& a, double* rmax, std::string* err) { return launch_row_lse_max_on(a, rmax, g_stream, err); }
int launch_ctc_viterbi_gaps_on(const ViterbiGapsArgs& a, hipStream_t stream, std::string* err);
int launch_ctc_viterbi_gaps(const ViterbiGapsArgs& a, std::string* err) { return launch_ctc_viterbi_gaps_on(a, g_stream, err); }
int launch_row_argmax_on(const RowLseArgs& a, int32_t* arg, int blank, hipStream_t stream, std::string* err);
int launch_row_argmax(const RowLseArgs& a, int32_t* arg, int blank, std::string* err) { return launch_row_argmax_on(a, arg, blank, g_stream, err); }
int launch_row_lse_argmax_on(const RowLseArgs& a, double* rmax, int32_t* arg, int blank, hipStream_t stream, std::string* err);
int launch_row_lse_argmax(const RowLseArgs& a, double* rmax, int32_t* arg, int blank, std::string* err) {
  return launch_row_lse_argmax_on(a, rmax, arg, blank, g_stream, err);
}
int launch_ctc_forward_ends_on(const ForwardArgs& a, const PrefixEnds* ends, int wave, hipStream_t stream, std::string* err);
int launch_ctc_forward_ends(const ForwardArgs& a, const PrefixEnds* ends, int wave, std::string* err) {
  return launch_ctc_forward_ends_on(a, ends, wave, g_stream, err);
}
int launch_ctc_prefix_extend_on(const PrefixExtendArgs& a, hipStream_t stream, std::string* err);
int launch_ctc_prefix_extend(const PrefixExtendArgs& a, std::string* err) { return launch_ctc_prefix_extend_on(a, g_stream, err); }
int launch_ctc_prefix_fill_on(double* next, const int32_t* rows, int32_t n_rows, int32_t V, hipStream_t stream, std::string* err);
int launch_ctc_prefix_fill(double* next, const int32_t* rows, int32_t n_rows, int32_t V, std::string* err) {
  return launch_ctc_prefix_fill_on(next, rows, n_rows, V, g_stream, err);
}
int launch_ctc_prefix_advance_on(const PrefixAdvanceArgs& a, hipStream_t stream, std::string* err);
int launch_ctc_prefix_advance(const PrefixAdvanceArgs& a, std::string* err) { return launch_ctc_prefix_advance_on(a, g_stream, err); }
int launch_greedy_collapse_on(const GreedyArgs& a, hipStream_t stream, std::string* err);
int launch_greedy_collapse(const GreedyArgs& a, std::string* err) { return launch_greedy_collapse_on(a, g_stream, err); }

// Survivor ledger, append (surv_ledger.h): one wavefront per stream. A step takes 64 of the chunk's rows, one per lane: the
// clamped counts are scanned across the wave (DPP, no LDS, no barrier), the running offset of the stream is wave-uniform and
// carried from step to step, every lane writes its row's end into row_off and copies its row's handful of (id, lp) pairs.
// Rows of one stream are contiguous in the strided arrays, so a step reads 64 consecutive counts and 64 rows max_surv entries
// apart, and writes one contiguous piece of the ledger. Plain vector stores throughout.
__global__ __launch_bounds__(64) void surv_ledger_append(LedgerAppendArgs a) {
  const uint32_t u = blockIdx.x, lane = threadIdx.x;
  const int64_t src0 = a.utt_row0[u];
  const uint32_t T = (uint32_t)(a.utt_row0[u + 1] - src0);
  const uint32_t r0 = a.led_row0[u];
  const uint32_t max_surv = (uint32_t)a.max_surv;
  uint64_t* ro = a.row_off + (size_t)u * (a.row_cap + 1);
  uint16_t* did = a.id + (size_t)u * a.ent_cap;
  double* dlp = a.lp + (size_t)u * a.ent_cap;
  if ((uint64_t)r0 + T > a.row_cap) {  // (the host reserved the rows: never)
    if (lane == 0) *a.overrun = 1;
    return;
  }
  uint64_t base = 0;  // wave-uniform: entries of the stream before the step's rows
  if (r0 == 0) {
    if (lane == 0) ro[0] = 0;
  } else {
    base = ro[r0];
  }
  bool bad = false;
  for (uint32_t t0 = 0; t0 < T; t0 += 64) {
    const uint32_t t = t0 + lane;
    const size_t src = (size_t)(src0 + t);
    const uint32_t cnt = t < T ? ledger_row_count(a.surv_cnt[src], max_surv) : 0u;
    const uint32_t incl = wave_incl_scan_u32(cnt);
    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    const uint64_t end = base + incl;
    if (t < T) {
      if (end <= a.ent_cap) {
        ro[(size_t)r0 + t + 1] = end;
        ledger_put_row(a.surv_id + src * max_surv, a.surv_lp + src * max_surv, cnt, did + (end - cnt), dlp + (end - cnt));
      } else {
        bad = true;
      }
    }
    base += total;
  }
  if (bad) *a.overrun = 1;  // (the host reserved the chunk's worst case: never)
  else if (lane == 0) a.used_out[u] = base;
}

template <int FOLD>
__global__ __launch_bounds__(256) void token_logp_ledger(LedgerLogpArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_tokens) return;
  const LedgerRun t = a.runs[i];
  double v;
  const uint32_t missing = ledger_logp_of<FOLD>(t, a.row_off + (size_t)t.stream * (a.row_cap + 1), a.id + (size_t)t.stream * a.ent_cap,
                                                a.lp + (size_t)t.stream * a.ent_cap, &v);
  a.out[i] = v;
  if (missing) atomicAdd(a.missing, missing);
}

static hipEvent_t g_led_ev[4] = {nullptr, nullptr, nullptr, nullptr};  // append start / end, fold start / end
static int ledger_events() {
  if (g_led_ev[0]) return 0;
  for (int k = 0; k < 4; ++k)
    if (hipEventCreate(&g_led_ev[k]) != hipSuccess) return -1;
  return 0;
}
static double ledger_ms(int k) {
  float ms = 0.f;
  if (!g_led_ev[k + 1] || hipEventSynchronize(g_led_ev[k + 1]) != hipSuccess) return 0.0;
  return hipEventElapsedTime(&ms, g_led_ev[k], g_led_ev[k + 1]) == hipSuccess ? (double)ms : 0.0;
}
int launch_ledger_append(const LedgerAppendArgs& a, std::string* err) {
  if (a.n_streams <= 0) return 0;
  HIP_TRY(ledger_events() ? hipErrorUnknown : hipSuccess);
  HIP_TRY(hipEventRecord(g_led_ev[0], g_stream));
  hipLaunchKernelGGL(surv_ledger_append, dim3((unsigned)a.n_streams), dim3(64), 0, g_stream, a);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(g_led_ev[1], g_stream));
  return 0;
}
int launch_ledger_logp(const LedgerLogpArgs& a, std::string* err) {
  if (a.n_tokens <= 0) return 0;
  HIP_TRY(ledger_events() ? hipErrorUnknown : hipSuccess);
  const dim3 grid((unsigned)((a.n_tokens + 255) / 256)), block(256);
  HIP_TRY(hipEventRecord(g_led_ev[2], g_stream));
  if (a.fold == LOGP_MEAN) hipLaunchKernelGGL(token_logp_ledger<LOGP_MEAN>, grid, block, 0, g_stream, a);
  else if (a.fold == LOGP_MIN) hipLaunchKernelGGL(token_logp_ledger<LOGP_MIN>, grid, block, 0, g_stream, a);
  else if (a.fold == LOGP_MAX) hipLaunchKernelGGL(token_logp_ledger<LOGP_MAX>, grid, block, 0, g_stream, a);
  else {
    if (err) *err = "unknown token_logp fold";
    return -1;
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(g_led_ev[3], g_stream));
  return 0;
}
double last_ledger_append_ms() { return ledger_ms(0); }
double last_ledger_logp_ms() { return ledger_ms(2); }

}  // namespace be
}  // namespace ctc
