// token_logp.h -- a token's confidence, folded over the frames of its run from the survivor lists the frame-prune stage
// left on the device ("Token confidences"). One body for the HIP kernel (backend_hip.hip: token_logp<FOLD>) and
// for the CPU simulator build, whose "device" memory is host memory (api.cpp under CTC_SIM).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "common.h"

namespace ctc {

// ctcdec_params.token_frames above 1: token frames plus this fold of the frames' log-probabilities
enum : int32_t { LOGP_MEAN = 2, LOGP_MIN = 3, LOGP_MAX = 4 };

// One token as the device sees it: `len` consecutive rows of the survivor arrays, starting at the absolute row `row`
// (utt_row0[u] + start), at each of which `label` was taken by the beam -- so it is among that row's survivors.
struct TokRun {  // 12 B
  uint32_t row, len, label;
};

// The fold of LP[f, label] over the run; mean = the sum in ascending frame order / len (the log of the geometric mean).
// Returns the number of frames whose survivor list does not hold the label: a broken invariant, the value is then void.
template <int FOLD>
CTC_HD uint32_t token_logp_of(const TokRun& t, const uint32_t* surv_cnt, const uint16_t* surv_id, const double* surv_lp,
                              uint32_t max_surv, double* out) {
  double acc = 0.0;
  uint32_t missing = 0;
  for (uint32_t f = 0; f < t.len; ++f) {
    const size_t row = (size_t)t.row + f;
    const uint32_t cnt = surv_cnt[row] < max_surv ? surv_cnt[row] : max_surv;
    const uint16_t* ids = surv_id + row * max_surv;
    uint32_t k = 0;
    while (k < cnt && ids[k] != t.label) ++k;
    if (k == cnt) {
      ++missing;
      continue;
    }
    const double lp = surv_lp[row * max_surv + k];
    if (FOLD == LOGP_MEAN) acc += lp;
    else if (FOLD == LOGP_MIN) acc = (f == 0 || lp < acc) ? lp : acc;
    else acc = (f == 0 || lp > acc) ? lp : acc;
  }
  *out = FOLD == LOGP_MEAN ? acc / (double)t.len : acc;
  return missing;
}

}  // namespace ctc
