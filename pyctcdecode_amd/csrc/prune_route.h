// prune_route.h -- which frame-prune kernel a call takes (host only: no HIP header, compiles with g++).
//
// prune_route() is the whole decision among the some seventy prune kernels of frame_prune_hip.hip, as a plain function of the
// call's shape that a test can ask (tests/test_prune_route.py): a wrong answer costs speed, every route computes the same.
#pragma once
#include <stdint.h>

namespace ctc {

// CTCDEC_PRUNE_EXP: how float32 rows sum their exponentials
enum PruneExp {
  PRUNE_EXP_NP = 0,   // (default) the reference's own float32 arithmetic: numpy's exp, summation order and log
  PRUNE_EXP_PK = 1,   // "pk": packed float32 polynomials, fp64 across the lanes
  PRUNE_EXP_F64 = 2,  // "f64": the fp64 exponential, per-row kernels only (diagnostics)
};
inline PruneExp prune_exp_of(const char* env) {
  return !env ? PRUNE_EXP_NP : env[0] == 'p' ? PRUNE_EXP_PK : env[0] == 'f' ? PRUNE_EXP_F64 : PRUNE_EXP_NP;
}
// CTCDEC_PRUNE_KERNEL=row: one wave per row for every row (diagnostics)
inline bool prune_per_row_forced(const char* env) { return env && env[0] == 'r'; }

struct PruneShape {
  int dtype;            // ctcdec_dtype: 0 float32, 1 float64, 2 float16, 3 bfloat16
  int n_labels;
  bool rows_aligned4;   // every row starts on a 4-byte boundary
  bool rows_aligned16;  // ... on a 16-byte boundary
  int pass;             // 0: logits; 1: the probability utterances again
  bool slow_list;       // the caller gave room for the list of rows the 64-rows-per-wave kernel hands over
  int64_t n_rows;
  bool dense_hint;      // most rows of the decoder's last calls came back on that list
  PruneExp exp;
  bool per_row_forced;
};

enum PruneKernel {
  PRUNE_FAST_F32,     // frame_prune_fast<nc, 0, al, np>
  PRUNE_FAST_16,      // frame_prune_fast<nc, dtype>
  PRUNE_ROW_F32X4,    // frame_prune_f32x4<nc, pk>
  PRUNE_ROW_GENERIC,  // frame_prune<T of dtype>
};
enum PruneListed {
  PRUNE_LISTED_NONE,
  PRUNE_LISTED_F32X4,    // frame_prune_f32x4_listed<nc>
  PRUNE_LISTED_GENERIC,  // frame_prune_listed<T of dtype>
};
struct PruneRoute {
  PruneKernel kernel;
  PruneListed listed;  // what runs the handed-over rows behind a fast kernel
  int nc;              // the instantiation's groups of four labels per lane (fast, f32x4)
  bool al;             // fast: 16-byte loads
  bool np;             // float32 rows in the reference's float32 arithmetic (PruneArgs::f32_np; the fast float32 kernel's NP)
  bool pk;             // f32x4: packed float32 exponentials
};

constexpr int PRUNE_FAST_MAX_LABELS = 4095;  // 64 lanes x 16 groups of four labels, less one: ids have to fit the 12-bit set tables

inline PruneRoute prune_route(const PruneShape& s) {
  const int V = s.n_labels;
  PruneRoute r{PRUNE_ROW_GENERIC, PRUNE_LISTED_NONE, 0, false, false, false};
  r.np = s.dtype == 0 && s.exp == PRUNE_EXP_NP;
  // The 64-rows-per-wave kernels hand rows over through the list, count them in 32 bits and have no fp64 exponential.
  // Vocabularies no larger than the survivor bound (character models, V ~ 30) take them too: peaky posteriors gain 35-40 % of
  // the stage; FLAT logits, where every row ends on the list, pay the screening on top of the per-row kernel (HISTORY.md 2.10)
  // until the caller notices and sets dense_hint (3.6 -> 1.8 ms) -- honoured only where both kernels give the same bits.
  const bool rows_ok = s.pass == 0 && s.slow_list && s.n_rows < (1ll << 32) && s.exp != PRUNE_EXP_F64 && !s.per_row_forced &&
                       !(s.dense_hint && r.np);
  if (s.dtype == 0 && V <= PRUNE_FAST_MAX_LABELS && s.rows_aligned4 && rows_ok) {
    // float32 rows of any label count and 4-byte alignment (16-byte loads when both allow them)
    const int nc = ((V + 3) / 4 + 63) / 64;  // groups of four labels per lane: 1 .. 16
    r.kernel = PRUNE_FAST_F32;
    r.nc = nc <= 8 ? nc : nc <= 12 ? 12 : 16;  // (groups past the row's end are masked)
    r.al = V % 4 == 0 && s.rows_aligned16;
    // the per-row float4 kernel where it applies (<= 1024 aligned labels), else the generic one
    r.listed = r.al && r.nc <= 4 ? PRUNE_LISTED_F32X4 : PRUNE_LISTED_GENERIC;
  } else if ((s.dtype == 2 || s.dtype == 3) && V % 8 == 0 && V <= 1024 && s.rows_aligned16 && rows_ok) {
    // 16-bit rows of a multiple of eight labels (16-byte loads of eight), widened on the fly
    r.kernel = PRUNE_FAST_16;
    r.nc = (V / 8 + 63) / 64 <= 1 ? 2 : 4;  // one 16-byte load per lane (up to 512 labels) or two
    r.al = true;
    r.listed = PRUNE_LISTED_GENERIC;
  } else if (s.dtype == 0 && V % 4 == 0 && V <= 1024 && s.rows_aligned16) {
    const int nc = (V / 4 + 63) / 64;
    r.kernel = PRUNE_ROW_F32X4;
    r.nc = nc <= 1 ? 1 : nc < 4 ? nc : 4;
    r.pk = s.exp != PRUNE_EXP_F64;
  }
  return r;
}

}  // namespace ctc
