// surv_ledger.h -- a device-resident stream's survivor ledger: what the frame prune decided for every frame pushed so far, kept
// so that a token's confidence can be folded over frames of earlier chunks ("Streaming tokens and confidences").
// The strided survivor arrays (surv_cnt / surv_id / surv_lp, max_surv entries per row) belong to one call and are overwritten
// by the next chunk; the ledger is their compact, grow-only copy in CSR form, per stream:
//   row_off[r] .. row_off[r + 1]   the entries of the stream's r-th frame (r counts from the stream's first frame)
//   id[k], lp[k]                   parallel arrays (uint16 labels, float64 log-probabilities: kept apart so that the doubles
//                                  stay 8-byte aligned), the first min(surv_cnt, max_surv) survivors of the row in prune order
// All streams of a handle share three allocations: stream u owns row_off[u * (row_cap + 1) ..], id / lp[u * ent_cap ..].
// One body for the HIP kernels (backend_hip.hip: surv_ledger_append, token_logp_ledger<FOLD>) and for the CPU simulator
// build, whose "device" memory is host memory (api.cpp under CTC_SIM).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "common.h"
#include "token_logp.h"

namespace ctc {

// One streamed token as the device sees it: `len` consecutive ledger rows of stream `stream`, starting at row `row`
// (the token's start frame - the stream's first frame), at each of which `label` was taken by the beam.
struct LedgerRun {  // 16 B
  uint32_t stream, row, len, label;
};

// entries a row of the strided arrays contributes: what the prune stage wrote of it
CTC_HD uint32_t ledger_row_count(uint32_t surv_cnt, uint32_t max_surv) { return surv_cnt < max_surv ? surv_cnt : max_surv; }

// one row's (id, lp) pairs to their place in the ledger
CTC_HD void ledger_put_row(const uint16_t* src_id, const double* src_lp, uint32_t cnt, uint16_t* dst_id, double* dst_lp) {
  for (uint32_t k = 0; k < cnt; ++k) {
    dst_id[k] = src_id[k];
    dst_lp[k] = src_lp[k];
  }
}

// token_logp_of (token_logp.h) over ledger rows: the same fold in the same order -- the mean is the float64 sum in ascending
// frame order divided by the count --, so a streamed token's value is bit for bit the one-shot decode's for the same frames.
// row_off / id / lp: the token's stream's own part of the ledger. Returns the number of frames whose row lacks the label.
template <int FOLD>
CTC_HD uint32_t ledger_logp_of(const LedgerRun& t, const uint64_t* row_off, const uint16_t* id, const double* lp, double* out) {
  double acc = 0.0;
  uint32_t missing = 0;
  for (uint32_t f = 0; f < t.len; ++f) {
    const size_t row = (size_t)t.row + f;
    const uint64_t end = row_off[row + 1];
    uint64_t k = row_off[row];
    while (k < end && id[k] != t.label) ++k;
    if (k == end) {
      ++missing;
      continue;
    }
    const double v = lp[k];
    if (FOLD == LOGP_MEAN) acc += v;
    else if (FOLD == LOGP_MIN) acc = (f == 0 || v < acc) ? v : acc;
    else acc = (f == 0 || v > acc) ? v : acc;
  }
  *out = FOLD == LOGP_MEAN ? acc / (double)t.len : acc;
  return missing;
}

}  // namespace ctc
