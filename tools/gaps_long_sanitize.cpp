// The body of ctc_viterbi_gaps_long under AddressSanitizer and UBSan, on the host: ctc_viterbi_gaps_long_utt (csrc/ctc_align.h)
// with a one-thread context on one small utterance whose every array is exactly as long as GapsLongUtt says, whole and at
// every segment length. An access outside any of them aborts. From the repository's root:
//   g++ -std=c++17 -O1 -g -DCTC_SIM -fsanitize=address,undefined -fno-omit-frame-pointer -Ipyctcdecode_amd/csrc \
//       tools/gaps_long_sanitize.cpp -o /tmp/gaps_long_sanitize && /tmp/gaps_long_sanitize
#include <stdio.h>

#include <vector>

#include "ctc_align.h"

using namespace ctc;

struct OneThread {
  int tid = 0, nt = 1;
  void sync() {}
};

int main() {
  const int V = 7, blank = 0, T = 23, L = 9;
  const int nch = align_chunks(L);
  std::vector<float> x((size_t)T * V);
  uint32_t seed = 12345u;
  for (float& v : x) v = (float)((seed = seed * 1664525u + 1013904223u) >> 24) / 32.0f - 4.0f;
  const std::vector<int32_t> lab = {3, 3, 5, 1, 6, 2, 2, 4, 1};
  const std::vector<uint8_t> gap = {1, 0, 0, 1, 0, 0, 1, 0, 0, 1};
  std::vector<double> lse(T), rmax(T);
  for (int t = 0; t < T; ++t) row_lse_max_seq(x.data(), 0, (size_t)t * V, V, false, &lse[t], &rmax[t]);
  std::vector<GapGroup> rec;
  for (int c = 0; c < nch; ++c) rec.push_back(gap_group_record(lab.data(), gap.data(), L, c));
  std::vector<int32_t> first_path;
  double first_score = 0;
  for (int K = T; K >= 1; --K) {
    const int n = align_long_segments(T, K);
    std::vector<double> col((size_t)8 * nch), ckpt((size_t)(n > 1 ? n : 0) * 4 * nch), tok_logp(L), gap_logp(L + 1), score(1);
    std::vector<uint8_t> bp((size_t)(K < T - 1 ? K : T - 1) * nch);
    std::vector<int32_t> path(T), tok_start(L), tok_end(L);
    GapsLongUtt u{x.data(), lse.data(), rmax.data(), lab.data(), gap.data(), rec.data(), col.data(), ckpt.data(), bp.data(), path.data(),
                  tok_start.data(), tok_end.data(), tok_logp.data(), gap_logp.data(), score.data(), T, L, 0, K};
    OneThread cx;
    ctc_viterbi_gaps_long_utt<0, GAPS_LONG_BATCH>(cx, u, V, blank, LOGP_MEAN, log(1e-15));
    if (K == T) first_path = path, first_score = score[0];
    if (path != first_path || score[0] != first_score) {
      printf("segments of %d frames: another path or score than the whole\n", K);
      return 1;
    }
  }
  printf("ctc_viterbi_gaps_long_utt: %d frames, %d labels, every segment length: score %.12f, clean\n", T, L, first_score);
  return 0;
}
