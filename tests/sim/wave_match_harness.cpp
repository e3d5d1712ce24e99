// wave_match_harness.cpp -- TEST INFRASTRUCTURE ONLY. A stand-alone program (tests/test_wave_match.py builds it with
// -fsanitize=address,undefined and runs it) that calls the wave kernel's hash match (beam_wave.h: wave_match) on 64 fibers
// (wave_fibers.h) with crafted key sets and compares rep[] with the brute-force "smallest valid index with an equal tag".
// Where a case is about one of the two routes -- the loser loop alone, or a second round on a cleared table first -- the
// number of table rounds the call reports is checked too. Prints one line per case; exit status 1 on any mismatch.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <cmath>
#include <vector>

#include "../../pyctcdecode_amd/csrc/beam_core.h"
#include "../../pyctcdecode_amd/csrc/beam_wave.h"
#include "wave_fibers.h"

namespace {

constexpr uint64_t TAG = ~127ull;
int g_failed = 0;

struct Set {
  std::vector<uint64_t> ck;   // [64 * A], candidate v
  std::vector<uint8_t> valid;
};

// a key that goes to slot s0 in round one and to slot s1 next, with `id` making its tag unlike any other's
uint64_t key_at(uint32_t s0, uint32_t s1, uint64_t id) {
  return ((uint64_t)(s0 & 127u) << 7) | ((uint64_t)(s1 & 127u) << 15) | (id << 23);
}

uint64_t rng_next(uint64_t& s) {
  s += 0x9E3779B97F4A7C15ull;
  uint64_t z = s;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

struct Case {
  const char* name;
  Set in;
  uint32_t want_rounds;  // 0: any
  bool quiet;
};

// all cases in one run of the 64 fibers (a run sets up 64 stacks: one per case would be most of the test's time)
template <int A>
void run_cases(const std::vector<Case>& cs, std::vector<uint32_t>& rep, std::vector<uint32_t>& ret) {
  alignas(16) static uint64_t table[128];
  rep.assign(cs.size() * 64 * A, 0);
  ret.assign(cs.size() * 64, 0);
  wavesim::Wave wave;
  wave.run([&](int lane) {
    wavesim::SimWaveCtx ctx{lane, &wave, nullptr, nullptr};
    for (size_t c = 0; c < cs.size(); ++c) {
      bool valid[A];
      uint64_t ck[A];
      uint32_t r[A];
      for (int j = 0; j < A; ++j) {
        valid[j] = cs[c].in.valid[j * 64 + lane] != 0;
        ck[j] = cs[c].in.ck[j * 64 + lane];
      }
      table[lane * 2] = table[lane * 2 + 1] = 0ull;  // (the caller clears the table)
      ctx.wsync();
      ret[c * 64 + lane] = ctc::wave_match<A, 128>(ctx, table, lane, valid, ck, r);
      for (int j = 0; j < A; ++j) rep[(c * A + j) * 64 + lane] = r[j];
      ctx.wsync();
    }
  });
}

template <int A>
void check_cases(const std::vector<Case>& cs) {
  std::vector<uint32_t> reps, rets;
  run_cases<A>(cs, reps, rets);
  for (size_t c = 0; c < cs.size(); ++c) {
    const Set& in = cs[c].in;
    const char* name = cs[c].name;
    const uint32_t* rep = &reps[c * 64 * A];
    const uint32_t* ret = &rets[c * 64];
    int bad = 0;
    for (int l = 1; l < 64; ++l)
      if (ret[l] != ret[0]) {
        printf("  %s A=%d: the lanes disagree on the round count (lane %d: %x, lane 0: %x)\n", name, A, l, ret[l], ret[0]);
        ++bad;
      }
    const uint32_t rounds = ret[0] & 0xFFFFu, steps = ret[0] >> 16;
    for (int v = 0; v < 64 * A; ++v) {
      uint32_t want = (uint32_t)v;
      if (in.valid[v])
        for (int u = 0; u < v; ++u)
          if (in.valid[u] && (in.ck[u] & TAG) == (in.ck[v] & TAG)) {
            want = (uint32_t)u;
            break;
          }
      if (rep[v] != want) {
        if (bad < 4) printf("  %s A=%d: candidate %d has rep %u, expected %u\n", name, A, v, rep[v], want);
        ++bad;
      }
    }
    if (cs[c].want_rounds && rounds != cs[c].want_rounds) {
      printf("  %s A=%d: %u table rounds, expected %u\n", name, A, rounds, cs[c].want_rounds);
      ++bad;
    }
    if (rounds > 2u) {
      printf("  %s A=%d: %u table rounds, never more than two\n", name, A, rounds);
      ++bad;
    }
    if (bad) ++g_failed;
    if (!cs[c].quiet || bad) printf("%s A=%d: %s (table rounds %u, loop steps %u)\n", name, A, bad ? "FAILED" : "ok", rounds, steps);
  }
}

template <int A>
Set empty_set() {
  Set s;
  s.ck.assign(64 * A, 0);
  s.valid.assign(64 * A, 0);
  return s;
}

// every candidate valid, each with a key of its own in a slot of its own (slots 1.., slot 0 is left to the case)
template <int A>
Set spread_set() {
  Set s = empty_set<A>();
  for (int v = 0; v < 64 * A; ++v) {
    s.valid[v] = 1;
    s.ck[v] = key_at(v < 127 ? (uint32_t)(v + 1) : 127u, (uint32_t)(v * 5 + 3), 1000 + (uint64_t)v);
  }
  if (A == 2) s.valid[127] = 0;  // (127 slots besides slot 0)
  return s;
}

template <int A>
void cases() {
  const int n = 64 * A;
  const int th = (int)ctc::WAVE_MATCH_LOOP_MAX;
  std::vector<Case> cs;
  {  // 1. all keys distinct, all in one round-one slot: one winner, 63 losers -> the round on the cleared table, then the loop
    Set s = empty_set<A>();
    for (int v = 0; v < 64; ++v) {
      s.valid[v] = 1;
      s.ck[v] = key_at(9, (uint32_t)(v % 11), 7 + (uint64_t)((v * 37) % 64));  // (second slots collide too)
    }
    cs.push_back({"1 one-slot", s, 2, false});
  }
  {  // 2. duplicates that both lose round one (a larger tag shares their slot): one pair, then five losers
    Set s = spread_set<A>();
    s.ck[3] = s.ck[17] = key_at(0, 40, 5);
    s.ck[30] = key_at(0, 41, 900);
    cs.push_back({"2 duplicates lose", s, 2 <= th ? 1u : 2u, false});
  }
  {
    Set s = spread_set<A>();
    s.ck[3] = s.ck[17] = s.ck[n - 2] = key_at(0, 40, 5);
    s.ck[8] = s.ck[9] = key_at(0, 40, 6);  // (and meets the first pair again in the next slot)
    s.ck[30] = key_at(0, 41, 900);          // the winner of slot 0
    cs.push_back({"2 more duplicates lose", s, 5 <= th ? 1u : 2u, false});
  }
  {  // 3. duplicates that win round one
    Set s = spread_set<A>();
    s.ck[5] = s.ck[6] = s.ck[n - 1] = key_at(0, 40, 900);
    s.valid[n - 1] = 1;
    s.ck[20] = key_at(0, 41, 5);
    s.ck[21] = s.ck[40] = key_at(0, 42, 6);
    cs.push_back({"3 duplicates win", s, 3 <= th ? 1u : 2u, false});
  }
  if (A == 2) {  // 4. a pair split across the two halves: once as winners, once as losers
    Set s = spread_set<A>();
    s.ck[5] = s.ck[64 + 9] = key_at(0, 40, 900);
    s.ck[12] = s.ck[64 + 12] = key_at(0, 41, 3);
    s.ck[64 + 30] = s.ck[31] = key_at(0, 41, 4);
    cs.push_back({"4 split pair", s, 4 <= th ? 1u : 2u, false});
  }
  // 5. the two sides of the threshold (WAVE_MATCH_LOOP_MAX and one more), and of the value it started from (8 and 9)
  const int counts[4] = {th, th + 1, 8, 9};
  const char* const names[4] = {"5 threshold losers", "5 threshold + 1 losers", "5 eight losers", "5 nine losers"};
  for (int c = 0; c < 4; ++c) {
    const int losers = counts[c];
    Set s = spread_set<A>();
    for (int k = 0; k <= losers; ++k) s.ck[(k * 7) % n] = key_at(0, (uint32_t)(50 + k % 3), 10 + (uint64_t)k);
    cs.push_back({names[c], s, losers <= th ? 1u : 2u, false});
  }
  {  // 6. partly invalid lanes: their keys equal valid ones and must neither be matched nor represent anything
    Set s = spread_set<A>();
    for (int v = 0; v < n; v += 3) s.valid[v] = 0;
    s.ck[0] = s.ck[1] = s.ck[4];               // 0 invalid, 1 and 4 valid
    s.ck[6] = s.ck[7];                         // 6 invalid
    s.ck[n - 4] = s.ck[n - 5] = key_at(0, 3, 77);
    s.ck[10] = s.ck[11] = key_at(0, 3, 78);
    cs.push_back({"6 invalid lanes", s, 0, false});
    Set none = empty_set<A>();
    cs.push_back({"6 no valid lane", none, 0, false});
  }
  {  // 7. seeded random sets, 0 - 30 % duplicates, dense and sparse tables
    uint64_t seed = 20260000u + (uint64_t)A;
    for (int it = 0; it < 1000; ++it) {
      Set s = empty_set<A>();
      const int nv = 1 + (int)(rng_next(seed) % (uint64_t)n);
      const uint64_t dup = rng_next(seed) % 31u;
      const bool crowded = (it % 5) == 4;  // few slots: many losers, the cleared-table round
      for (int v = 0; v < nv; ++v) {
        s.valid[v] = 1;
        if (v > 0 && rng_next(seed) % 100u < dup) s.ck[v] = s.ck[rng_next(seed) % (uint64_t)v];
        else s.ck[v] = crowded ? key_at((uint32_t)(rng_next(seed) % 6u), (uint32_t)(rng_next(seed) % 9u), rng_next(seed) >> 24) : rng_next(seed);
      }
      for (int v = nv; v < n; ++v) s.ck[v] = s.ck[rng_next(seed) % (uint64_t)nv];  // (invalid lanes carry somebody's key)
      cs.push_back({"7 random", s, 0, true});
    }
  }
  check_cases<A>(cs);
  printf("7 random A=%d: 1000 sets done\n", A);
}

}  // namespace

int main() {
  cases<1>();
  cases<2>();
  printf(g_failed ? "FAILED: %d cases\n" : "all cases ok\n", g_failed);
  return g_failed ? 1 : 0;
}
