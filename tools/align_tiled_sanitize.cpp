// The bodies of ctc_viterbi_tile and ctc_viterbi_cone under AddressSanitizer and UBSan, on the host: ctc_viterbi_tile_body over
// every live tile in diagonal order, then ctc_viterbi_cone_utt (csrc/ctc_align.h), with a one-thread context on small utterances
// whose every array is exactly as long as AlignTiledUtt and align_tiled_plan say, at the library's own tile shape and at the
// shapes of the tests; each result against ctc_viterbi_long_utt's. An access outside any array aborts. From the repository's root:
//   g++ -std=c++17 -O1 -g -DCTC_SIM -fsanitize=address,undefined -fno-omit-frame-pointer -Ipyctcdecode_amd/csrc \
//       tools/align_tiled_sanitize.cpp -o /tmp/align_tiled_sanitize && /tmp/align_tiled_sanitize
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "ctc_align.h"

using namespace ctc;

struct OneThread {
  enum { GROUPS = FORWARD_TILE_MAX_GROUPS };
  int tid = 0, nt = 1;
  void sync() {}
};

struct Result {
  std::vector<int32_t> path, tok_start, tok_end;
  std::vector<double> tok_logp;
  double score = 0;
  bool operator==(const Result& o) const {
    return path == o.path && tok_start == o.tok_start && tok_end == o.tok_end && tok_logp == o.tok_logp && score == o.score;
  }
};

static const int V = 7, BLANK = 0;

static Result untiled(const std::vector<float>& x, const std::vector<double>& lse, const std::vector<int32_t>& lab, int T) {
  const int L = (int)lab.size(), nch = align_chunks(L);
  Result r{std::vector<int32_t>(T), std::vector<int32_t>(L), std::vector<int32_t>(L), std::vector<double>(L), 0};
  std::vector<double> col((size_t)8 * nch);
  std::vector<uint8_t> bp((size_t)T * nch);
  AlignLongUtt u{x.data(), lse.data(), lab.data(), col.data(), nullptr, bp.data(), r.path.data(), r.tok_start.data(), r.tok_end.data(),
                 r.tok_logp.data(), &r.score, T, L, 0, T};
  OneThread cx;
  ctc_viterbi_long_utt(cx, u, V, 0, BLANK, LOGP_MEAN, log(1e-15));
  return r;
}

static Result tiled(const std::vector<float>& x, const std::vector<double>& lse, const std::vector<int32_t>& lab, int T, const int* cut) {
  const int L = (int)lab.size(), nch = align_chunks(L);
  const AlignTiledPlan pl = align_tiled_plan(T, L, 0, cut[0], cut[1], cut[2]);
  Result r{std::vector<int32_t>(T), std::vector<int32_t>(L), std::vector<int32_t>(L), std::vector<double>(L), 0};
  std::vector<double> col((size_t)4 * nch, align_neg_inf()), edge((size_t)FORWARD_TILE_RING * (pl.nI - 1) * pl.FB, align_neg_inf()),
      ckpt((size_t)(pl.n - 1) * 4 * nch, align_neg_inf()), lds((size_t)2 * FORWARD_TILE_MAX_GROUPS);
  if (8 * (int64_t)(col.size() + edge.size() + ckpt.size()) != pl.bytes) printf("the plan's bytes are not the arrays'\n"), exit(1);
  std::vector<uint8_t> bp((size_t)ALIGN_TILED_BP_BYTES);
  int32_t s_end = -1;
  int hand = 0;
  AlignTiledUtt u{x.data(), lse.data(), lab.data(), col.data(), edge.data(), ckpt.data(), &s_end, r.path.data(), r.tok_start.data(),
                  r.tok_end.data(), r.tok_logp.data(), &r.score, T, L, 0, pl.GB, pl.FB, pl.KB};
  OneThread cx;
  for (int d = 0; d < pl.nI + pl.nJ - 1; ++d)
    for (int i = 0; i < pl.nI; ++i)
      if (d - i >= 0 && d - i < pl.nJ && forward_tile_live(T, L, pl.GB, pl.FB, i, d - i))
        ctc_viterbi_tile_body<0>(cx, u, i, d - i, viterbi_tile_keep(T, pl.FB, pl.KB, d - i), V, BLANK, log(1e-15), lds.data());
  ctc_viterbi_cone_utt<0>(cx, u, V, BLANK, LOGP_MEAN, log(1e-15), lds.data(), bp.data(), &hand);
  return r;
}

int main() {
  const int cuts[][3] = {{0, 0, 0}, {1, 1, 1}, {3, 5, 2}, {2, 7, 1}, {256, 64, 7}, {100, 97, 2}};
  uint32_t seed = 12345u;
  const auto next = [&] { return (seed = seed * 1664525u + 1013904223u) >> 24; };
  // (frames, labels): at the feasibility bound, a few groups, more than a thousand frames in segments of 448
  const int shapes[][2] = {{1, 0}, {1, 1}, {12, 12}, {23, 9}, {300, 129}, {1000, 300}};
  for (const auto& sh : shapes) {
    const int T = sh[0], L = sh[1];
    std::vector<float> x((size_t)T * V);
    for (float& v : x) v = (float)next() / 32.0f - 4.0f;
    std::vector<int32_t> lab(L);
    for (int k = 0; k < L; ++k) lab[k] = 1 + (int)(next() % (V - 1));
    for (int k = 1; k < L; ++k)
      if (lab[k] == lab[k - 1]) lab[k] = 1 + lab[k] % (V - 1);  // (no repeats: T >= L suffices)
    std::vector<double> lse(T);
    for (int t = 0; t < T; ++t) lse[t] = row_lse_seq(x.data(), 0, (size_t)t * V, V);
    const Result want = untiled(x, lse, lab, T);
    for (const auto& cut : cuts)
      if (!(tiled(x, lse, lab, T, cut) == want)) {
        printf("%d frames, %d labels, tiles (%d, %d, %d): another result than ctc_viterbi_long_utt's\n", T, L, cut[0], cut[1], cut[2]);
        return 1;
      }
    printf("%d frames, %d labels: %d tile shapes equal to ctc_viterbi_long_utt, score %.12f, clean\n", T, L, (int)(sizeof cuts / sizeof *cuts),
           want.score);
  }
  return 0;
}
