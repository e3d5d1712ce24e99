// api_internal.h -- what the translation units behind include/ctcdec.h share: api.cpp (the beam decode, streams, results) and
// api_transcript.cpp (the calls on known transcripts). Nothing here is part of the library's interface.
#pragma once
#include <stdint.h>
#include <stddef.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/ctcdec.h"
#include "backend.h"
#include "host_tables.h"

// Shared between the two files, not with the library's users: kept out of its exports.
#define CTC_INTERNAL __attribute__((visibility("hidden")))

using namespace ctc;

// The calling thread's message for ctcdec_last_error; returns `code`.
CTC_INTERNAL int fail(int code, const std::string& msg);
// Calls that touch the device are serialised (api.cpp).
CTC_INTERNAL extern std::mutex g_device_mu;

using Clock = std::chrono::steady_clock;
static inline double ms(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }
static inline size_t dtype_size(int32_t dtype) { return dtype == CTCDEC_F32 ? 4 : dtype == CTCDEC_F64 ? 8 : 2; }

// Grow-only device (HOST: page-locked staging) memory, owned: released with the buffer, handed over by a move.
template <bool HOST>
struct Buf {
  void* p = nullptr;
  size_t cap = 0;
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  Buf(Buf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  Buf& operator=(Buf&& o) noexcept {  // (what this held goes to `o`, and away with it)
    std::swap(p, o.p);
    std::swap(cap, o.cap);
    return *this;
  }
  ~Buf() { drop(); }
  CTC_INTERNAL int ensure(size_t bytes, std::string* err) {
    if (bytes <= cap && p) return 0;
    drop();
    const size_t want = HOST ? bytes + bytes / 4 + 4096 : bytes + bytes / 8 + 256;
    p = HOST ? be::alloc_host(want, err) : be::alloc(want, err);
    if (!p) return -1;
    cap = want;
    return 0;
  }
  CTC_INTERNAL void drop() {
    if (p) HOST ? be::release_host(p) : be::release(p);
    p = nullptr;
    cap = 0;
  }
};
using DevBuf = Buf<false>;
using HostBuf = Buf<true>;

template <class T>
CTC_INTERNAL int upload(DevBuf& b, const std::vector<T>& v, std::string* err) {
  size_t bytes = std::max<size_t>(sizeof(T) * v.size(), 16);
  if (b.ensure(bytes, err)) return -1;
  if (!v.empty() && be::h2d(b.p, v.data(), sizeof(T) * v.size(), err)) return -1;
  return 0;
}

// A few persistent host threads for the per-utterance replay (spawning them per call cost more than the
// work itself: 8 x ~80 us on the bench box). Jobs are index ranges handed out through an atomic cursor.
class ReplayPool {
 public:
  explicit ReplayPool(int n) {
    for (int i = 0; i < n; ++i) workers_.emplace_back([this] { loop(); });
  }
  ~ReplayPool() {
    {
      std::lock_guard<std::mutex> g(m_);
      stop_ = true;
    }
    cv_.notify_all();
    for (auto& t : workers_) t.join();
  }
  int size() const { return (int)workers_.size(); }
  // fn(u0, u1) over [0, n) in chunks; returns when all chunks are done (the caller works too)
  void run(int32_t n, int32_t chunk, const std::function<void(int32_t, int32_t)>& fn) {
    {
      std::lock_guard<std::mutex> g(m_);
      fn_ = &fn;
      n_ = n;
      chunk_ = chunk;
      next_.store(0);
      pending_ = (int)workers_.size();
      ++epoch_;
    }
    cv_.notify_all();
    work();
    std::unique_lock<std::mutex> g(m_);
    done_.wait(g, [this] { return pending_ == 0; });
    fn_ = nullptr;
  }

 private:
  void work() {
    for (;;) {
      int32_t u0 = next_.fetch_add(chunk_);
      if (u0 >= n_) return;
      (*fn_)(u0, std::min(n_, u0 + chunk_));
    }
  }
  void loop() {
    uint64_t seen = 0;
    for (;;) {
      {
        std::unique_lock<std::mutex> g(m_);
        cv_.wait(g, [&] { return stop_ || epoch_ != seen; });
        if (stop_) return;
        seen = epoch_;
      }
      work();
      {
        std::lock_guard<std::mutex> g(m_);
        if (--pending_ == 0) done_.notify_one();
      }
    }
  }
  std::vector<std::thread> workers_;
  std::mutex m_;
  std::condition_variable cv_, done_;
  const std::function<void(int32_t, int32_t)>* fn_ = nullptr;
  std::atomic<int32_t> next_{0};
  int32_t n_ = 0, chunk_ = 1;
  int pending_ = 0;
  uint64_t epoch_ = 0;
  bool stop_ = false;
};

struct ctcdec_decoder {
  std::unique_ptr<ReplayPool> replay_pool;  // created on the first large batch
  HostAlphabet alpha;
  std::shared_ptr<HostLM> lm_ptr = std::make_shared<HostLM>();
  HostLM& lm_ref() { return *lm_ptr; }
  const HostLM& lm_ref() const { return *lm_ptr; }
  bool has_lm = false;
  // MultiLanguageModel: lm_ptr is model 0, multi holds all of them plus the union tables
  std::unique_ptr<HostMulti> multi;
  double x_alpha[MAX_LMS] = {0}, x_beta[MAX_LMS] = {0}, x_unk[MAX_LMS] = {0};
  int32_t x_boundary[MAX_LMS] = {0};
  int n_lms() const { return multi ? (int)multi->lms.size() : 1; }
  int hist_order() const { return multi ? multi->order : lm_ptr->order; }
  HostHotwords hot;
  bool tables_dirty = true, hot_dirty = true;
  // per-utterance hot words (ctcdec_set_hotword_sets): armed for the next decode call only. That call moves them to
  // hot_call (HotCallScope) and builds the sets' tables when it first needs them; they are gone when it returns.
  struct HotSets {
    bool armed = false;
    std::vector<std::vector<std::string>> words;  // per set: its unigrams
    std::vector<double> weight;
    std::vector<int32_t> utt_set;                 // per utterance / stream: its set (-1: none)
    bool built = false;
    std::vector<HostHotwords> sets;               // words.size() sets, plus an empty one when some utterance has none
  };
  HotSets hot_next, hot_call;
  DevBuf d_hsets, d_htab, d_htok, d_hutt;
  HostBuf h_hot;
  DevBuf d_tok, d_tok_hot, d_uni, d_pref, d_hot;  // (the n-gram tables: NgramStore::device, shared between decoders)
  DevBuf d_xuni[MAX_LMS - 1], d_winfo[MAX_LMS], w_xstate, w_impx;
  HostBuf h_xstate;
  // per-call workspace (grow only)
  DevBuf w_logits, w_ptrs, w_row0, w_rowsum, w_isprob, w_scnt, w_sid, w_slp, w_flags, w_text, w_emit, w_toff,
      w_eoff, w_start, w_out, w_nout, w_status, w_tok, w_head, w_prof, w_imp, w_impoff, w_ff, w_cold, w_pay, w_tscr, w_tsoff, w_tpool,
      d_toktext, d_tokbytes, w_slow, w_order, w_side, w_truns, w_tlogp, w_tmiss, w_ledrow;
  // forced alignment (ctcdec_align_batch): row log-sum-exps, targets, paths, token spans, confidences, scores, the launch's
  // back-pointer tables and utterance records
  DevBuf w_alse, w_alab, w_apath, w_atok, w_atlp, w_ascore, w_abp, w_autts;
  // forced alignment of long transcripts (ctcdec_align_long_batch): a launch's score columns, checkpoints and utterance
  // records (the segment tables: w_abp; everything else: the alignment's)
  DevBuf w_lcol, w_lckpt, w_lutts;
  // transcript likelihood (ctcdec_score_batch): the hypothesis records of a launch (labels: w_alab, scores: w_ascore)
  DevBuf w_fhyps;
  // frame posteriors (ctcdec_posteriors_batch): a launch's tables and utterance records, the token sums (labels: w_alab,
  // score pairs: w_ascore)
  DevBuf w_ptab, w_putts, w_pocc;
  // transcript gradient (ctcdec_gradient_batch): the labels' occurrence lists, a launch's row records and, for host callers,
  // its gradient rows (tables, labels and scores: the posteriors')
  DevBuf w_gocc, w_gutts, w_grad;
  // phrase search (ctcdec_find_batch): a launch's traces and phrase records, the call's hits (labels: w_alab)
  DevBuf w_ftrace, w_fphr, w_fhits;
  // alignment with gaps (ctcdec_align_gaps_batch): row maxima, the slots' gap flags, the gaps' sums, a launch's utterance
  // records (everything else: the alignment's)
  DevBuf w_amax, w_agap, w_aglp, w_agutts;
  // greedy decode (ctcdec_greedy_batch): the rows' labels, the utterances' token counts and offsets, the tokens' labels, spans
  // and confidences (row maxima: w_amax, scores: w_ascore)
  DevBuf w_garg, w_gcnt, w_gtoff, w_glab, w_gspan, w_glogp;
  // prefix scores (ctcdec_prefix_batch): the end states and scales the forward pass stores, their records in launch order
  // and by prefix, the prefixes' last labels, the chunks, a split launch's sums, the rows without a launch and, for host
  // callers, the result (labels: w_alab, scores: w_ascore, hypothesis records: w_fhyps). A prefix session's calls use the
  // same ones for a step's records, and w_fhyps for its children's
  DevBuf w_xends, w_xscale, w_xrecl, w_xrech, w_xlast, w_xchunks, w_xpart, w_xrows, w_xnext;
  bool slicing = false;  // a time-sliced host ingest is under way (decode_host_sliced): the prune stage notes each slice's side of 1
  uint32_t max_label_bytes = 1;
  bool arenas_worst_case = false;  // a call has outgrown the usual reservation of the node arenas: reserve the worst case from now on
  HostBuf h_tok, h_out, h_small, h_truns;
  int dense_calls = 0;      // calls left that skip the 64-rows-per-wave prune kernel (most rows of a recent call overflowed it)
  HostBuf h_stage;          // page-locked staging of a call's small uploads (upload_staged): they go over without the host waiting
  size_t stage_used = 0;
  bool profile = false;
  unsigned long long prof[N_PROF] = {0};
};

// The frame-prune stage of a call: what it runs on, and what it reports.
struct PruneStage {
  ctcdec_decoder* dec = nullptr;
  const std::vector<const void*>* ptrs = nullptr;  // the utterances' device pointers (already uploaded to w_ptrs, like w_row0)
  int32_t n_utts = 0, dtype = 0;
  int64_t R = 0;  // frames of all utterances
  int V = 0;
  double token_min_logp = 0;
  bool resident = false;   // resident streams do not take the dense_calls hint (nor does the diagnostic, which leaves it alone)
  int max_surv = 0;        // out: the width of the survivor lists the stage ended with
  uint32_t flags[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // out: PruneArgs::overflow as last read
  uint32_t surv_total = 0;                       // out: flags[4] of the last pass
  Clock::time_point t_setup, t_queued, t_flags;  // (CTCDEC_HOST_TIMING: where the host side of a call goes)
};

struct DecodeCall;
// The frame-prune stage (api.cpp, inside its extern "C" block). `beam`: the decode whose beam stage reads the lists, or nullptr.
extern "C" CTC_INTERNAL int prune_stage(PruneStage& s, DecodeCall* beam);
