// api.cpp -- the C ABI of include/ctcdec.h on top of backend.h + host_tables.h.
#include <math.h>
#include <cmath>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <memory>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "api_internal.h"
#include "../../include/ctcdec.h"
#include "backend.h"
#include "beam_core.h"
#include "beam_wave.h"
#include "host_tables.h"

using namespace ctc;

static thread_local std::string g_err;
// The backend owns one stream and one set of timing events per process: calls that touch the device are
// serialised (several host threads may share decoders; the GIL is released during ctypes calls).
std::mutex g_device_mu;
int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

namespace {

struct BeamResult {
  std::string text;
  std::vector<int32_t> word_off, start, end;
  double logit = 0, lm = 0;
  ctcdec_lm_state state;
  std::vector<ctcdec_lm_state> xstates;  // MultiLanguageModel: states of model 1..
  // streaming extras (decoder.py:69-79 fields of the returned LMBeam)
  std::string partial;
  int32_t src = -1, last_char = -1, pstart = -1, pend = -1;
  double raw_lm = 0;
  // params.token_frames: (label, start, end) of every token of the beam, root to leaf (replay())
  std::vector<int32_t> tok;
};

// what a streaming call adds to a plain batch decode
struct StreamIn {
  const int32_t* first_frame;
  const ctcdec_beam_in* beams;
  const int64_t* beam_off;
  const char* text_blob;
  int32_t fold, eos;
};

}  // namespace

// A call's small per-utterance tables (pointers, row offsets, arena offsets, start states): copied into the decoder's page-locked
// staging block and sent on the decode stream WITHOUT waiting -- the kernels that read them are queued behind them on the same
// stream. (upload() waits for every copy: six round trips of ~20 us in front of the first kernel of a call.) The block is reused
// from the start by the next call, which begins after this one's last synchronisation. Falls back to upload() when it is full.
template <class T>
static int upload_staged(ctcdec_decoder* dec, DevBuf& b, const std::vector<T>& v, std::string* err) {
  const size_t bytes = sizeof(T) * v.size();
  const size_t room = dec->h_stage.p ? dec->h_stage.cap - dec->stage_used : 0;
  if (bytes == 0 || bytes > room) return upload(b, v, err);
  if (b.ensure(std::max<size_t>(bytes, 16), err)) return -1;
  char* src = (char*)dec->h_stage.p + dec->stage_used;
  memcpy(src, v.data(), bytes);
  dec->stage_used += (bytes + 63) & ~(size_t)63;
  return be::h2d_async(b.p, src, bytes, err);
}

// The sets armed by ctcdec_set_hotword_sets belong to the one decode call that takes them: moved into hot_call for
// the call's duration, dropped when it returns (whatever its outcome).
struct HotCallScope {
  ctcdec_decoder* dec;
  explicit HotCallScope(ctcdec_decoder* d) : dec(d) {
    if (!dec) return;
    dec->hot_call = std::move(dec->hot_next);
    dec->hot_next = ctcdec_decoder::HotSets();
  }
  ~HotCallScope() {
    if (dec) dec->hot_call = ctcdec_decoder::HotSets();
  }
};

// the host tables of the call's sets (HostHotwords::build_table: the same hash and min_len / complete rules as the
// call-wide set); utterances without a set are pointed at a trailing empty one
static void build_hot_sets(ctcdec_decoder::HotSets& h) {
  if (h.built) return;
  h.sets.resize(h.words.size());
  for (size_t k = 0; k < h.words.size(); ++k) h.sets[k].build_table(h.words[k]);
  bool none = false;
  for (int32_t& s : h.utt_set) {
    if (s < 0) {
      s = (int32_t)h.words.size();
      none = true;
    }
  }
  if (none) {
    h.sets.emplace_back();
    h.weight.push_back(0.0);
  }
  h.built = true;
}

// hot-word table a streaming import of stream u resolves its beams' words against
static const HostHotwords& import_hot(const ctcdec_decoder* dec, int64_t u) {
  const ctcdec_decoder::HotSets& h = dec->hot_call;
  return h.armed ? h.sets[(size_t)h.utt_set[(size_t)u]] : dec->hot;
}

// Upload the call's sets: their tables one behind the other, one per-label view of n_labels entries per set (filled by the
// device: be::launch_beam), the descriptors and each utterance's set index -- copied from page-locked memory on the decode
// stream without the host waiting (the kernels that read them are queued behind). Sets ba's hot-set fields.
static int upload_hot_sets(ctcdec_decoder* dec, be::BeamArgs* ba, std::string* err) {
  ctcdec_decoder::HotSets& h = dec->hot_call;
  build_hot_sets(h);
  const size_t K = h.sets.size(), V = dec->alpha.labels.size(), n = h.utt_set.size();
  std::vector<size_t> toff(K + 1, 0);
  for (size_t k = 0; k < K; ++k) toff[k + 1] = toff[k] + h.sets[k].table.size();
  const size_t b_sets = K * sizeof(HotSet), b_utt = n * sizeof(int32_t), b_tab = toff[K] * sizeof(HotEntry);
  const size_t o_utt = (b_sets + 63) & ~(size_t)63, o_tab = (o_utt + b_utt + 63) & ~(size_t)63;
  if (dec->d_hsets.ensure(std::max<size_t>(b_sets, 16), err) || dec->d_hutt.ensure(std::max<size_t>(b_utt, 16), err) ||
      dec->d_htab.ensure(std::max<size_t>(b_tab, 16), err) || dec->d_htok.ensure(std::max<size_t>(K * V * sizeof(TokHot), 16), err) ||
      dec->h_hot.ensure(o_tab + b_tab + 64, err))
    return -1;
  char* stage = (char*)dec->h_hot.p;
  HotSet* hs = (HotSet*)stage;
  for (size_t k = 0; k < K; ++k) {
    const HostHotwords& w = h.sets[k];
    hs[k].hot = w.table.empty() ? nullptr : (const HotEntry*)dec->d_htab.p + toff[k];
    hs[k].hot_mask = w.mask;
    hs[k].tok_hot = (const TokHot*)dec->d_htok.p + k * V;
    hs[k].weight = h.weight[k];
    if (!w.table.empty()) memcpy(stage + o_tab + toff[k] * sizeof(HotEntry), w.table.data(), w.table.size() * sizeof(HotEntry));
  }
  memcpy(stage + o_utt, h.utt_set.data(), b_utt);
  if (be::h2d_async(dec->d_hsets.p, stage, b_sets, err) || be::h2d_async(dec->d_hutt.p, stage + o_utt, b_utt, err) ||
      (b_tab && be::h2d_async(dec->d_htab.p, stage + o_tab, b_tab, err)))
    return -1;
  ba->hot_sets = (const HotSet*)dec->d_hsets.p;
  ba->utt_hot = (const int32_t*)dec->d_hutt.p;
  ba->n_hot_sets = (int32_t)K;
  return 0;
}

struct ctcdec_result {
  std::vector<std::vector<BeamResult>> utts;
  double ms[3] = {0, 0, 0};
  int beam_kernel = 0;  // be::last_beam_kernel() of the launch that produced this result
  // texts only (ctcdec_result_texts)
  bool texts_packed = false;
  std::string t_blob;
  std::vector<int64_t> t_off;
  std::string j_blob;  // ctcdec_result_texts_joined
  // params.texts_only: the texts as the device wrote them (one block per utterance somewhere in dev_texts) and the
  // output records; BeamResults are only built when an accessor other than ctcdec_result_texts_joined asks for them
  bool device_texts = false;
  std::string dev_texts;
  std::vector<OutBeam> dev_out;  // [n_utts]
  std::vector<int64_t> blk_off, blk_len;  // ctcdec_result_text_blocks
  // packed view (built on demand by ctcdec_result_pack)
  bool packed = false;
  std::vector<int64_t> beam_off, text_off, word_cnt_off;
  std::string text_blob;
  std::vector<double> logit, lm;
  std::vector<int32_t> word_byte_off, word_start, word_end;
  std::vector<ctcdec_lm_state> states;
  std::string partial_blob;
  std::vector<int64_t> partial_off;
  std::vector<int32_t> src_beam, last_char, pstart, pend;
  std::vector<double> raw_lm;
  // token frames (params.token_frames; packed by ctcdec_result_token_frames in the order of ctcdec_result_pack)
  bool has_tokens = false, tok_packed = false;
  std::vector<int64_t> tk_off;
  std::vector<int32_t> tk_label, tk_start, tk_end;
  // token confidences (params.token_frames = CTCDEC_TOKEN_LOGP_*), in the same order: filled by the decode call itself
  bool has_logp = false;
  std::vector<double> tk_logp;
};

// A batch of device-resident streams (ctcdec_stream_*): what survives between chunks lives in device memory owned by
// the handle -- per stream a row of carried beams (the ImportBeam records the kernels' finalisation writes and the next
// chunk's import_beams() reads), the emission arena (grow-only: the chains reach back to the start of the stream) and
// the counters -- plus host mirrors of the counters, refreshed after every push.
struct ctcdec_stream {
  ctcdec_decoder* dec = nullptr;
  int32_t n = 0;
  int K = 1;
  static constexpr int CAP = CTCDEC_MAX_BEAM_WIDTH;  // carried beams per stream
  DevBuf carry, carry_x, sstate, emit, eoff;
  uint64_t emit_cap = 0;  // emission nodes per stream
  std::vector<StreamState> mirror;
  std::vector<int64_t> frames;  // frames pushed so far
  int64_t pushes = 0;           // chunks pushed since the streams' last start (each may close a word: one more chain entry)
  std::vector<ctcdec_lm_state> start_states;  // n * K, or empty: the models' defaults
  // the caller's beams of the last ctcdec_stream_import: roots (BR_IMPORT) of the chains decoded since
  bool has_import = false;
  std::vector<ctcdec_beam_in> imp_beams;
  std::vector<int64_t> imp_off;
  std::string imp_blob;
  // The survivor ledger (surv_ledger.h), only for streams whose first push asked for a confidence fold (led_fold != 0):
  // what the frame prune left for every frame pushed so far, CSR per stream, grow-only like the emission arena. The
  // entries each stream holds come back with the counters after every push (they ride behind them in `sstate`:
  // n StreamStates, n entry counts, the overrun word).
  int32_t led_fold = 0;
  DevBuf led_off, led_id, led_lp;
  uint64_t led_row_cap = 0, led_ent_cap = 0;  // rows / entries per stream
  std::vector<uint64_t> led_used;             // entries per stream after the last push
  std::vector<int32_t> led_first;             // first_frame of each stream's first chunk: ledger row = frame - led_first
  std::vector<uint64_t> led_back;             // host side of the widened counter read
  size_t sstate_bytes() const { return (size_t)n * sizeof(StreamState); }
  size_t led_bytes() const { return led_off.cap + led_id.cap + led_lp.cap; }
};

// the device copy of a model's n-gram table: uploaded once per NgramStore, shared by every decoder that holds the model
// or a clone of it, released with the last of them
static const NgramEntry* device_ngrams(const HostLM& lm) {
  return lm.ngr->device ? (const NgramEntry*)static_cast<DevBuf*>(lm.ngr->device.get())->p : nullptr;
}
static int upload_ngrams(const HostLM& lm, std::string* err) {
  if (lm.ngr->device) return 0;
  auto buf = std::make_shared<DevBuf>();
  if (upload(*buf, lm.ngr->table, err)) return -1;
  lm.ngr->device = buf;
  return 0;
}

static int sync_tables(ctcdec_decoder* d, std::string* err) {
  if (d->tables_dirty) {
    if (d->multi) fill_token_starts_from(d->multi->prefix_table, d->multi->prefix_mask, &d->alpha);
    else if (d->has_lm) d->lm_ref().fill_token_starts(&d->alpha);
    if (upload(d->d_tok, d->alpha.tok, err)) return -1;
    {  // the labels' UTF-8 bytes, for the kernels that assemble texts themselves
      std::vector<TokText> tt(d->alpha.labels.size());
      std::string bytes;
      uint32_t longest = 1;
      for (size_t i = 0; i < tt.size(); ++i) {
        const std::string &raw = d->alpha.labels[i], &clean = d->alpha.clean[i];
        tt[i].raw_off = (uint32_t)bytes.size();
        tt[i].raw_len = (uint16_t)raw.size();
        bytes += raw;
        tt[i].clean_off = (uint32_t)bytes.size();
        tt[i].clean_len = (uint16_t)clean.size();
        bytes += clean;
        tt[i].pad = 0;
        longest = std::max<uint32_t>(longest, (uint32_t)std::max(raw.size(), clean.size()));
      }
      std::vector<uint8_t> bv(bytes.begin(), bytes.end());
      if (bv.empty()) bv.push_back(0);
      if (upload(d->d_toktext, tt, err) || upload(d->d_tokbytes, bv, err)) return -1;
      d->max_label_bytes = longest;
    }
    if (d->has_lm) {
      if (upload(d->d_uni, d->lm_ref().unigrams, err)) return -1;
      if (upload_ngrams(d->lm_ref(), err)) return -1;
      if (upload(d->d_pref, d->multi ? d->multi->prefix_table : d->lm_ref().prefix_table, err)) return -1;
    }
    if (d->multi) {
      for (int k = 0; k < d->n_lms(); ++k) {
        if (upload(d->d_winfo[k], d->multi->winfo[(size_t)k], err)) return -1;
        if (k > 0 && (upload(d->d_xuni[k - 1], d->multi->lms[(size_t)k]->unigrams, err) ||
                      upload_ngrams(*d->multi->lms[(size_t)k], err)))
          return -1;
      }
    }
    d->tables_dirty = false;
    d->hot_dirty = true;
  }
  if (d->hot_dirty) {
    if (d->hot.tok_hot.size() != d->alpha.tok.size()) d->hot.build({}, d->alpha);
    if (upload(d->d_tok_hot, d->hot.tok_hot, err)) return -1;
    if (upload(d->d_hot, d->hot.table, err)) return -1;
    d->hot_dirty = false;
  }
  return 0;
}

// a kernel-side LM state as the ABI hands it out
static void export_lm_state(const LmState& s, ctcdec_lm_state* out) {
  out->length = s.len;
  for (int k = 0; k < MAX_CTX; ++k) {
    out->words[k] = s.words[k];
    out->backoff[k] = s.backoff[k];
  }
}

static void device_tables(const ctcdec_decoder* d, DeviceTables* t) {
  memset(t, 0, sizeof(*t));
  if (d->has_lm) d->lm_ref().tables(t);
  t->tok = (const TokInfo*)d->d_tok.p;
  t->tok_hot = (const TokHot*)d->d_tok_hot.p;
  t->tok_text = (const TokText*)d->d_toktext.p;
  t->tok_bytes = (const uint8_t*)d->d_tokbytes.p;
  t->max_label_bytes = d->max_label_bytes;
  if (d->has_lm) {
    t->unigrams = (const UnigramEntry*)d->d_uni.p;
    t->ngrams = device_ngrams(d->lm_ref());
    t->prefixes = (const PrefixEntry*)d->d_pref.p;
    if (d->multi) {
      t->prefix_mask = d->multi->prefix_mask;
      t->n_lms = (uint32_t)d->n_lms();
      t->n_hist = (uint32_t)std::max(1, d->multi->order - 1);
      t->winfo0 = (const uint32_t*)d->d_winfo[0].p;
      for (int k = 1; k < d->n_lms(); ++k) {
        const HostLM& lm = *d->multi->lms[(size_t)k];
        LmExtra& x = t->x[k - 1];
        x.unigrams = (const UnigramEntry*)d->d_xuni[k - 1].p;
        x.ngrams = device_ngrams(*d->multi->lms[(size_t)k]);
        x.ngram_mask = lm.ngram_mask;
        x.winfo = (const uint32_t*)d->d_winfo[k].p;
        x.lm_order = (uint32_t)lm.order;
        x.has_trie = lm.has_trie ? 1u : 0u;
        x.uniset_nonempty = lm.uniset_size > 0 ? 1u : 0u;
        x.eos_id = lm.eos_id;
        x.alpha = d->x_alpha[k];
        x.beta = d->x_beta[k];
        x.unk = d->x_unk[k];
        x.score_boundary = d->x_boundary[k];
      }
    }
  } else {
    t->n_hist = 1;  // lm_order 1 without an LM (decoder.py:551)
  }
  t->hot = d->hot.table.empty() ? nullptr : (const HotEntry*)d->d_hot.p;
  t->hot_mask = d->hot.mask;
  t->n_labels = (uint32_t)d->alpha.labels.size();
  t->is_bpe = d->alpha.is_bpe ? 1u : 0u;
}

extern "C" {

const char* ctcdec_last_error(void) { return g_err.c_str(); }
const char* ctcdec_version(void) { return "ctcdec 0.1 (gfx950)"; }

int ctcdec_create(const char* labels_blob, const int64_t* labels_off, int32_t n_labels, int32_t is_bpe,
                  int32_t device, ctcdec_decoder** out) {
  if (!labels_blob || !labels_off || !out || n_labels <= 0) return fail(CTCDEC_ERR_ARG, "bad arguments");
  if (n_labels > CTCDEC_MAX_VOCAB) return fail(CTCDEC_ERR_LIMIT, "vocabulary larger than 65535 labels");
  std::string err;
  if (be::init(device, &err)) return fail(CTCDEC_ERR_DEVICE, err);
  std::unique_ptr<ctcdec_decoder> d(new ctcdec_decoder());
  std::vector<std::string> labels;
  for (int32_t i = 0; i < n_labels; ++i)
    labels.emplace_back(labels_blob + labels_off[i], (size_t)(labels_off[i + 1] - labels_off[i]));
  d->alpha.build(labels, is_bpe != 0);
  d->hot.build({}, d->alpha);
  *out = d.release();
  return CTCDEC_OK;
}

void ctcdec_destroy(ctcdec_decoder* dec) { delete dec; }

int ctcdec_lm_load_arpa(ctcdec_decoder* dec, const char* path, int32_t* order_out) {
  if (!dec || !path) return fail(CTCDEC_ERR_ARG, "bad arguments");
  std::string e = dec->lm_ref().load_arpa(path);
  if (!e.empty()) return fail(CTCDEC_ERR_IO, e);
  dec->has_lm = true;
  dec->tables_dirty = true;
  if (order_out) *order_out = dec->lm_ref().order;
  return CTCDEC_OK;
}

int ctcdec_lm_save_flat(const ctcdec_decoder* dec, const char* path) {
  if (!dec || !path || !dec->has_lm) return fail(CTCDEC_ERR_ARG, "no language model loaded");
  std::string e = dec->lm_ref().save_cache(path);
  if (!e.empty()) return fail(CTCDEC_ERR_IO, e);
  return CTCDEC_OK;
}

int ctcdec_lm_load_flat(ctcdec_decoder* dec, const char* path, int32_t* order_out) {
  if (!dec || !path) return fail(CTCDEC_ERR_ARG, "bad arguments");
  if (dec->multi) return fail(CTCDEC_ERR_ARG, "decoder holds several language models");
  std::string e = dec->lm_ref().load_cache(path);
  if (!e.empty()) return fail(CTCDEC_ERR_IO, e);
  dec->has_lm = true;
  dec->tables_dirty = true;
  if (order_out) *order_out = dec->lm_ref().order;
  return CTCDEC_OK;
}

int ctcdec_lm_load_kenlm(ctcdec_decoder* dec, const char* path, int32_t* order_out) {
  if (!dec || !path) return fail(CTCDEC_ERR_ARG, "bad arguments");
  if (dec->multi) return fail(CTCDEC_ERR_ARG, "decoder holds several language models");
  std::string e = dec->lm_ref().load_kenlm_binary(path);
  if (!e.empty()) return fail(CTCDEC_ERR_IO, e);
  dec->has_lm = true;
  dec->tables_dirty = true;
  if (order_out) *order_out = dec->lm_ref().order;
  return CTCDEC_OK;
}

int ctcdec_is_kenlm_binary(const char* path) { return path && looks_like_kenlm_binary(path) ? 1 : 0; }

int ctcdec_arpa_to_kenlm_binary(const char* arpa_path, const char* out_path, float probing_multiplier) {
  if (!arpa_path || !out_path) return fail(CTCDEC_ERR_ARG, "bad arguments");
  std::string e = arpa_to_kenlm_binary(arpa_path, out_path, probing_multiplier);
  if (!e.empty()) return fail(CTCDEC_ERR_IO, e);
  return CTCDEC_OK;
}

int ctcdec_lm_set_unigrams(ctcdec_decoder* dec, int32_t has_unigrams, const char* blob, const int64_t* off,
                           int64_t n_unigrams, int64_t* n_kept_out) {
  if (!dec || !dec->has_lm) return fail(CTCDEC_ERR_ARG, "no language model loaded");
  std::vector<std::string> uni;
  if (has_unigrams)
    for (int64_t i = 0; i < n_unigrams; ++i) uni.emplace_back(blob + off[i], (size_t)(off[i + 1] - off[i]));
  dec->lm_ref().set_unigrams(has_unigrams != 0, uni);
  dec->tables_dirty = true;
  if (n_kept_out) *n_kept_out = (int64_t)dec->lm_ref().uniset_size;
  return CTCDEC_OK;
}

int ctcdec_lm_share(ctcdec_decoder* dst, const ctcdec_decoder* src) {
  if (!dst || !src || !src->has_lm) return fail(CTCDEC_ERR_ARG, "source has no language model");
  if (src->multi) return fail(CTCDEC_ERR_ARG, "source holds several language models");
  dst->lm_ptr = src->lm_ptr;
  dst->multi.reset();
  dst->has_lm = true;
  dst->tables_dirty = true;
  return CTCDEC_OK;
}

int ctcdec_lm_clone(ctcdec_decoder* dst, const ctcdec_decoder* src) {
  if (!dst || !src || !src->has_lm) return fail(CTCDEC_ERR_ARG, "source has no language model");
  if (src->multi) return fail(CTCDEC_ERR_ARG, "source holds several language models");
  dst->lm_ptr = std::make_shared<HostLM>(*src->lm_ptr);  // own tables: own unigram set, own prefix flags
  dst->multi.reset();
  dst->has_lm = true;
  dst->tables_dirty = true;
  return CTCDEC_OK;
}

int ctcdec_lm_share_multi(ctcdec_decoder* dst, const ctcdec_decoder* const* srcs, int32_t n) {
  if (!dst || !srcs || n < 2) return fail(CTCDEC_ERR_ARG, "a MultiLanguageModel holds at least 2 language models");
  if (n > CTCDEC_MAX_LMS) return fail(CTCDEC_ERR_LIMIT, "more language models than CTCDEC_MAX_LMS");
  std::unique_ptr<HostMulti> m(new HostMulti());
  for (int32_t k = 0; k < n; ++k) {
    if (!srcs[k] || !srcs[k]->has_lm || srcs[k]->multi) return fail(CTCDEC_ERR_ARG, "source has no (single) language model");
    m->lms.push_back(srcs[k]->lm_ptr);
  }
  m->build();
  if (m->words.size() > WI_ID_MASK) return fail(CTCDEC_ERR_LIMIT, "union vocabulary too large");
  dst->lm_ptr = m->lms[0];
  dst->multi = std::move(m);
  dst->has_lm = true;
  dst->tables_dirty = true;
  return CTCDEC_OK;
}

int ctcdec_lm_set_params(ctcdec_decoder* dec, int32_t k, double alpha, double beta, double unk_score_offset,
                         int32_t lm_score_boundary) {
  if (!dec || !dec->multi || k < 1 || k >= dec->n_lms()) return fail(CTCDEC_ERR_ARG, "no such additional language model");
  dec->x_alpha[k] = alpha;
  dec->x_beta[k] = beta;
  dec->x_unk[k] = unk_score_offset;
  dec->x_boundary[k] = lm_score_boundary ? 1 : 0;
  return CTCDEC_OK;
}

int ctcdec_lm_count(const ctcdec_decoder* dec, int32_t* n_out) {
  if (!dec || !n_out) return fail(CTCDEC_ERR_ARG, "bad arguments");
  *n_out = dec->has_lm ? dec->n_lms() : 0;
  return CTCDEC_OK;
}

int ctcdec_lm_prefix_flags(const ctcdec_decoder* dec, const char* s, int64_t len, uint32_t* flags_out) {
  if (!dec || !dec->has_lm || !flags_out) return fail(CTCDEC_ERR_ARG, "no language model loaded");
  uint32_t wid = 0, fl = 0;
  const HostLM& lm = dec->lm_ref();
  *flags_out = 0;
  if (len > 0 && prefix_lookup(lm.prefix_table.data(), lm.prefix_mask, hash_bytes(s, (size_t)len), &wid, &fl))
    *flags_out = fl;
  return CTCDEC_OK;
}

int ctcdec_lm_word_index(const ctcdec_decoder* dec, const char* w, int64_t len, uint32_t* index_out) {
  if (!dec || !dec->has_lm || !index_out) return fail(CTCDEC_ERR_ARG, "no language model loaded");
  *index_out = dec->lm_ref().index(std::string(w, (size_t)len));
  return CTCDEC_OK;
}

int ctcdec_lm_word_string(const ctcdec_decoder* dec, uint32_t index, const char** str_out, int64_t* len_out) {
  if (!dec || !dec->has_lm || index >= dec->lm_ref().words.size()) return fail(CTCDEC_ERR_ARG, "bad word index");
  *str_out = dec->lm_ref().words[index].data();
  *len_out = (int64_t)dec->lm_ref().words[index].size();
  return CTCDEC_OK;
}

int ctcdec_lm_start_state(const ctcdec_decoder* dec, int32_t begin_sentence, ctcdec_lm_state* out) {
  if (!dec || !dec->has_lm || !out) return fail(CTCDEC_ERR_ARG, "no language model loaded");
  LmState st;
  dec->lm_ref().start_state(begin_sentence != 0, &st);
  export_lm_state(st, out);
  return CTCDEC_OK;
}

int ctcdec_lm_base_score(const ctcdec_decoder* dec, const ctcdec_lm_state* in, uint32_t word_index,
                         ctcdec_lm_state* out, float* log10_prob_out) {
  if (!dec || !dec->has_lm || !in || !out || !log10_prob_out) return fail(CTCDEC_ERR_ARG, "bad arguments");
  if (word_index >= dec->lm_ref().words.size() || in->length < 0 || in->length > MAX_CTX)
    return fail(CTCDEC_ERR_ARG, "bad LM state or word index");
  DeviceTables t;
  dec->lm_ref().tables(&t);
  LmState a, b;
  a.len = in->length;
  for (int k = 0; k < MAX_CTX; ++k) {
    a.words[k] = in->words[k];
    a.backoff[k] = in->backoff[k];
  }
  *log10_prob_out = lm_base_score(t, a, word_index, &b);
  export_lm_state(b, out);
  return CTCDEC_OK;
}

int ctcdec_set_hotwords(ctcdec_decoder* dec, const char* blob, const int64_t* off, int64_t n_words) {
  if (!dec) return fail(CTCDEC_ERR_ARG, "bad arguments");
  std::string err;
  std::lock_guard<std::mutex> device_lock(g_device_mu);
  if (be::bind_thread(&err)) return fail(CTCDEC_ERR_DEVICE, err);
  std::vector<std::string> uni;
  for (int64_t i = 0; i < n_words; ++i) uni.emplace_back(blob + off[i], (size_t)(off[i + 1] - off[i]));
  dec->hot.build(uni, dec->alpha);
  dec->hot_dirty = true;
  return CTCDEC_OK;
}

int ctcdec_set_hotword_sets(ctcdec_decoder* dec, const char* blob, const int64_t* off, int64_t n_words, const int64_t* set_off,
                            int32_t n_sets, const double* set_weight, const int32_t* utt_set, int32_t n_utts) {
  if (!dec) return fail(CTCDEC_ERR_ARG, "bad arguments");
  dec->hot_next = ctcdec_decoder::HotSets();
  if (n_words < 0 || n_sets < 0 || n_utts < 0 || (n_words > 0 && (!blob || !off)) || (n_sets > 0 && (!set_off || !set_weight)) ||
      (n_utts > 0 && !utt_set))
    return fail(CTCDEC_ERR_ARG, "bad arguments");
  // the kernels of the HIP backend take each utterance's set; a backend that does not must not decode them with another
  if (strncmp(be::name(), "hip", 3) != 0)
    return fail(CTCDEC_ERR_LIMIT, std::string("per-utterance hot words are not supported by the '") + be::name() + "' backend");
  if (n_sets > 0 && (set_off[0] != 0 || set_off[n_sets] != n_words)) return fail(CTCDEC_ERR_ARG, "set_off must run from 0 to n_words");
  ctcdec_decoder::HotSets h;
  h.words.resize((size_t)n_sets);
  h.weight.assign(set_weight, set_weight + n_sets);
  for (int32_t k = 0; k < n_sets; ++k) {
    if (set_off[k + 1] < set_off[k]) return fail(CTCDEC_ERR_ARG, "set_off must not decrease");
    if (!std::isfinite(set_weight[k])) return fail(CTCDEC_ERR_ARG, "hot-word weights must be finite");
    for (int64_t i = set_off[k]; i < set_off[k + 1]; ++i) {
      if (off[i + 1] < off[i]) return fail(CTCDEC_ERR_ARG, "bad word offsets");
      h.words[(size_t)k].emplace_back(blob + off[i], (size_t)(off[i + 1] - off[i]));
    }
  }
  h.utt_set.assign(utt_set, utt_set + n_utts);
  for (int32_t s : h.utt_set)
    if (s < -1 || s >= n_sets) return fail(CTCDEC_ERR_ARG, "utterance set index out of range");
  h.armed = true;
  dec->hot_next = std::move(h);
  return CTCDEC_OK;
}

// Rebuild text + word frames of one beam from its emission list (root -> leaf). The text is written
// in place: `open` is where the currently open (partial) word starts. A streaming beam starts from the
// caller's beam named by its BR_IMPORT root (text so far + open partial word).
// want_tok: the same pass also lists the beam's tokens with their frames ("Token frames"). An APPEND node
// holds 1 + its own start frame; a BOUNDARY token's start is the start of the word it opens, which the next word-closing
// node carries (or, for the last word, open_s: the beam's open-word frames the kernel leaves in OutBeam::pad). Every
// node holds the end of the token before it in wend (partial_frames[1], decoder.py:449-534); the last token's end is
// open_e. Space labels of a character alphabet (BR_SPACE) are separators and are not listed.
static void replay(const ctcdec_decoder* d, const EmitNode* toks, uint32_t n, const StreamIn* st, int64_t imp0,
                   BeamResult* r, bool want_tok = false, int32_t open_s = -1, int32_t open_e = -1) {
  constexpr size_t NONE = ~(size_t)0;
  std::vector<int32_t>& tk = r->tok;
  size_t last = NONE, opener = NONE;  // the token whose end / BOUNDARY token whose start the next node gives
  if (want_tok) {
    tk.clear();
    tk.reserve((size_t)n * 3);
  }
  std::string& text = r->text;
  text.clear();
  text.reserve((size_t)n * 3 + 8);
  size_t open = 0;
  auto close_word = [&](int32_t s, int32_t e, bool more) {
    if (text.size() == open) return;  // empty open word: nothing to close
    r->word_off.push_back((int32_t)open);
    r->start.push_back(s);
    r->end.push_back(e);
    if (more) text.push_back(' ');
    open = text.size();
  };
  for (uint32_t k = 0; k < n; ++k) {
    const uint32_t br = toks[k].tok_branch >> 16, tok = toks[k].tok_branch & 0xFFFFu;
    if (want_tok) {
      if (br == BR_IMPORT) {  // (streaming: the tokens before the caller's beam are not on this chain)
        last = opener = NONE;
      } else {
        if (last != NONE) tk[last * 3 + 2] = toks[k].wend;
        last = NONE;
        if (br != BR_APPEND && opener != NONE) {
          tk[opener * 3 + 1] = toks[k].wstart;
          opener = NONE;
        }
        if (br == BR_BOUNDARY || br == BR_APPEND) {
          last = tk.size() / 3;
          if (br == BR_BOUNDARY) opener = last;
          tk.push_back((int32_t)tok);
          tk.push_back(br == BR_APPEND ? toks[k].wstart - 1 : -1);
          tk.push_back(-1);
        }
      }
    }
    if (br == BR_BOUNDARY) {
      close_word(toks[k].wstart, toks[k].wend, true);
      text += d->alpha.clean[tok];
    } else if (br == BR_SPACE) {
      close_word(toks[k].wstart, toks[k].wend, true);
    } else if (br == BR_APPEND) {
      text += d->alpha.labels[tok];
    } else if (br == BR_FINAL) {
      // (the last entry of a folded beam, or -- resident streams after force_next_word -- an entry in the middle of
      // the chain: the trailing separator of the former is dropped below)
      close_word(toks[k].wstart, toks[k].wend, true);
    } else if (br == BR_IMPORT && st) {
      const ctcdec_beam_in& in = st->beams[imp0 + tok];
      r->src = (int32_t)tok;
      text.assign(st->text_blob + in.text_begin, (size_t)(in.text_end - in.text_begin));
      if (!text.empty()) text.push_back(' ');
      open = text.size();
      text.append(st->text_blob + in.partial_begin, (size_t)(in.partial_end - in.partial_begin));
    }
  }
  if (want_tok) {
    if (last != NONE) tk[last * 3 + 2] = open_e;
    if (opener != NONE) tk[opener * 3 + 1] = open_s;
  }
  // split off the still open word (streaming without force_next_word / is_end)
  r->partial.assign(text, open, std::string::npos);
  text.resize(open);
  if (!text.empty() && text.back() == ' ') text.pop_back();
  r->word_off.push_back((int32_t)text.size());
}

// OutBeam record (+ the states of the further language models) -> the host-side beam; the text follows by replay()
static void fill_result(const OutBeam& ob, const LmState* xs, int K, BeamResult* r) {
  r->logit = ob.logit_score;
  r->lm = ob.lm_score;
  export_lm_state(ob.state, &r->state);
  if (xs) {
    r->xstates.resize((size_t)(K - 1));
    for (int x = 0; x < K - 1; ++x) export_lm_state(xs[x], &r->xstates[(size_t)x]);
  }
  r->last_char = ob.last_char == NO_CHAR ? -1 : (int32_t)ob.last_char;
  r->pstart = ob.pstart;
  r->pend = ob.pend;
  r->raw_lm = ob.raw_lm;
}

// the fold of a call that asks for token confidences (ctcdec_params.token_frames = CTCDEC_TOKEN_LOGP_*), else 0
static_assert(LOGP_MEAN == CTCDEC_TOKEN_LOGP_MEAN && LOGP_MIN == CTCDEC_TOKEN_LOGP_MIN && LOGP_MAX == CTCDEC_TOKEN_LOGP_MAX, "token_logp.h");
static int32_t logp_fold(const ctcdec_params* p) {
  return p && p->token_frames >= LOGP_MEAN && p->token_frames <= LOGP_MAX ? p->token_frames : 0;
}

// A caller's LM state into the kernels' form: its length must lie in [0, MAX_CTX], every word index below the model's word count.
enum LmStateErr { LM_STATE_OK = 0, LM_STATE_LENGTH, LM_STATE_WORD };
static LmStateErr copy_lm_state(const ctcdec_lm_state& in, size_t n_words, LmState* out) {
  memset(out, 0, sizeof(*out));
  if (in.length < 0 || in.length > MAX_CTX) return LM_STATE_LENGTH;
  out->len = in.length;
  for (int j = 0; j < out->len; ++j) {
    if (in.words[j] >= n_words) return LM_STATE_WORD;
    out->words[j] = in.words[j];
    out->backoff[j] = in.backoff[j];
  }
  return LM_STATE_OK;
}

typedef std::function<int(std::string*)> AfterLaunch;
// How a decode call is run. Neither pointer: a plain batch. `stream` alone: host imports. `rs`: the streams are device-
// resident (`stream` then only carries first_frame / fold / eos and, below an import, the caller's beams for the replay).
struct DecodeMode {
  const StreamIn* stream = nullptr;
  ctcdec_stream* rs = nullptr;
  bool want_result = true;  // materialise beams at all (a resident stream between reads: no)
  // called once the kernels of this call are queued and before the host waits for them (time-sliced host ingest: the next
  // slice's copy runs under this slice's kernels)
  const AfterLaunch* after_launch = nullptr;
};
static int decode_impl(ctcdec_decoder* dec, const void* const* utt_logits, const int32_t* utt_frames, int32_t n_utts,
                       int32_t dtype, int32_t is_device, const ctcdec_params* p, const ctcdec_lm_state* start_states,
                       const DecodeMode& mode, ctcdec_result** out);
static int decode_host_sliced(ctcdec_decoder* dec, const void* const* utt_logits, const int32_t* utt_frames, int32_t n_utts,
                              int32_t dtype, const ctcdec_params* p, const ctcdec_lm_state* start_states, int n_slices,
                              ctcdec_result** out);
static int host_slices_wanted(const ctcdec_decoder* dec, const int32_t* utt_frames, int32_t n_utts, int32_t dtype);

int ctcdec_decode_batch(ctcdec_decoder* dec, const void* const* utt_logits, const int32_t* utt_frames,
                        int32_t n_utts, int32_t dtype, int32_t is_device, const ctcdec_params* p,
                        const ctcdec_lm_state* start_states, ctcdec_result** out) {
  HotCallScope hot_scope(dec);
  // Large HOST batches (the reference's own calling convention: numpy in) go over in time slices, the copy of slice k + 1
  // under the kernels of slice k (decode_host_sliced); 1 = "decode it in one piece after all" (probability-like rows).
  // (per-utterance hot words: in one piece)
  // (token confidences: in one piece too -- a slice's survivor lists are overwritten by the next slice's)
  if (dec && p && out && !is_device && !dec->hot_call.armed && !logp_fold(p) && n_utts > 0 && utt_logits && utt_frames && dtype >= CTCDEC_F32 && dtype <= CTCDEC_BF16) {
    const int n_slices = host_slices_wanted(dec, utt_frames, n_utts, dtype);
    if (n_slices >= 2) {
      const int rc = decode_host_sliced(dec, utt_logits, utt_frames, n_utts, dtype, p, start_states, n_slices, out);
      if (rc != 1) return rc;
    }
  }
  return decode_impl(dec, utt_logits, utt_frames, n_utts, dtype, is_device, p, start_states, DecodeMode(), out);
}

int ctcdec_decode_stream_batch(ctcdec_decoder* dec, const void* const* utt_logits, const int32_t* utt_frames,
                               int32_t n_streams, int32_t dtype, int32_t is_device, const ctcdec_params* p,
                               const int32_t* first_frame, const ctcdec_beam_in* beams, const int64_t* beam_off,
                               const char* text_blob, int32_t force_next_word, int32_t is_end, ctcdec_result** out) {
  if (!first_frame || !beams || !beam_off || !text_blob) return fail(CTCDEC_ERR_ARG, "bad arguments");
  const StreamIn st{first_frame, beams, beam_off, text_blob, (force_next_word || is_end) ? 1 : 0, is_end ? 1 : 0};
  HotCallScope hot_scope(dec);
  return decode_impl(dec, utt_logits, utt_frames, n_streams, dtype, is_device, p, nullptr, DecodeMode{&st}, out);
}

// host side of a streaming import: strings -> hashes, table views, history ring (the kernel rebuilds
// the beam row and its TextNode from this)
static std::string build_import(const ctcdec_decoder* dec, const StreamIn& st, int64_t k, ImportBeam* m,
                                LmState* more /* n_lms - 1 entries, or nullptr */, const HostHotwords& hot) {
  const ctcdec_beam_in& in = st.beams[k];
  memset(m, 0, sizeof(*m));
  if (in.text_end < in.text_begin || in.partial_end < in.partial_begin) return "bad beam text range";
  const char* t = st.text_blob + in.text_begin;
  const size_t tn = (size_t)(in.text_end - in.text_begin);
  const uint32_t n_hist = dec->has_lm ? (uint32_t)std::max(1, dec->hist_order() - 1) : 1u;
  uint64_t th = 0;
  std::vector<uint64_t> wh;
  uint32_t hw = 0;
  size_t a = 0;
  while (a < tn) {
    while (a < tn && t[a] == ' ') ++a;
    size_t b = a;
    while (b < tn && t[b] != ' ') ++b;
    if (b > a) {
      uint64_t h = hash_bytes(t + a, b - a);
      th = text_push(th, h);
      wh.push_back(h);
      uint32_t ml = 0, cp = 0;
      if (!hot.table.empty() && hot_lookup(hot.table.data(), hot.mask, h, &ml, &cp) && cp) ++hw;
    }
    a = b;
  }
  m->text_h = th;
  m->hw_cnt = hw;
  m->ring_cnt = (uint32_t)std::min<size_t>(n_hist, wh.size());
  for (uint32_t j = 0; j < m->ring_cnt; ++j) m->ring[j] = wh[wh.size() - 1 - j];
  const char* pp = st.text_blob + in.partial_begin;
  const size_t pn = (size_t)(in.partial_end - in.partial_begin);
  m->part_h = hash_bytes(pp, pn);
  m->plen = utf8_length(pp, pn);
  if (m->plen > 0xFFFF) return "partial word too long";
  uint32_t m2 = 0, wid = 0;
  if (pn > 0) {
    uint32_t fl = 0, w = 0;
    const std::vector<PrefixEntry>& ptab = dec->multi ? dec->multi->prefix_table : dec->lm_ref().prefix_table;
    const uint64_t pmask = dec->multi ? dec->multi->prefix_mask : dec->lm_ref().prefix_mask;
    if (dec->has_lm && prefix_lookup(ptab.data(), pmask, m->part_h, &w, &fl)) {
      m2 |= PF_ON_TABLE | (fl & PF_PARTIAL_MASK);
      wid = w;
    }
    uint32_t ml = 0, cp = 0;
    if (!hot.table.empty() && hot_lookup(hot.table.data(), hot.mask, m->part_h, &ml, &cp))
      m2 |= M2_HOT_ON | (cp ? M2_HOT_COMPLETE : 0u) | ((ml & 0xFFFFu) << 8);
  }
  m->m2 = m2;
  m->word_id = wid;
  if (in.last_char >= (int32_t)dec->alpha.labels.size()) return "last_char out of range";
  m->last_char = in.last_char < 0 ? NO_CHAR : (uint32_t)in.last_char;
  m->pstart = in.partial_start;
  m->pend = in.partial_end_frame;
  m->logit_score = in.logit_score;
  m->raw_lm = dec->has_lm ? in.raw_lm_score : 0.0;
  const char* const bad_state[] = {nullptr, "bad LM state in beam", "bad LM state word in beam"};
  if (dec->has_lm) {
    if (const LmStateErr e = copy_lm_state(in.lm_state, dec->lm_ref().words.size(), &m->state)) return bad_state[e];
  }
  if (dec->multi) {
    if (!in.more_states) return "beam lacks the states of the further language models";
    for (int x = 1; x < dec->n_lms(); ++x)
      if (const LmStateErr e = copy_lm_state(in.more_states[x - 1], dec->multi->lms[(size_t)x]->words.size(), &more[x - 1]))
        return bad_state[e];
  }
  return "";
}

// ---- one decode call, stage by stage: decode_impl is a short driver over the stages below, which share one DecodeCall ----

struct DecodeCall : DecodeMode {
  ctcdec_decoder* dec = nullptr;
  const ctcdec_params* p = nullptr;
  const void* const* utt_logits = nullptr;
  const int32_t* utt_frames = nullptr;
  const ctcdec_lm_state* start_states = nullptr;
  ctcdec_result** out = nullptr;
  int32_t n_utts = 0, dtype = 0, is_device = 0, fold = 0;
  int V = 0, K = 1, B = 0, n_best = 0;
  int64_t R = 0;
  std::vector<int64_t> row0;
  std::vector<const void*> ptrs;
  std::vector<uint64_t> toff, eoff;  // node offsets of the text / emission arenas
  bool arenas_full = false;
  unsigned long long tok_cap = 0;
  size_t xstate_bytes = 0;
  bool device_texts = false, by_input = false, late_beam = false;
  be::BeamArgs ba{};
  PruneStage prune;
  // the counters of the beam stage, in page-locked memory (h_small)
  uint32_t *n_out = nullptr, *status = nullptr;
  unsigned long long* heads_pinned = nullptr;
  unsigned long long head = 0;
  bool outgrown_redone = false;
  // resident streams: the fold of the streams' survivor ledger when this call appends to it (0: the streams keep none),
  // the rows each stream's ledger holds once this chunk is in, the streams' first frames
  int32_t led = 0;
  std::vector<int64_t> led_rows;
  bool host_timing = false;
  Clock::time_point t_begin, t_launch, t_kernel, t_end;
  std::string err;
  std::unique_ptr<ctcdec_result> res;
  std::unique_lock<std::mutex> device_lock;  // (last: released first)
};

// Tokens and confidences of a device-resident stream, refused before anything moves. The chains of a stream reach back to its
// start unless the host imported its beams; the survivor ledger exists only when the stream's first push asked for a fold, and
// its rows are numbered from the first frame of that push, so every later chunk has to continue where the last one ended.
static int check_stream_tokens(DecodeCall& c) {
  const ctcdec_stream* rs = c.rs;
  if (c.p->token_frames != 0 && rs->has_import)
    return fail(CTCDEC_ERR_ARG, "token frames are not available to a stream that holds imported beams: their chains do not reach back");
  const bool first = rs->pushes == 0;  // (a new stream, or the first chunk after is_end)
  if (c.fold && !first && rs->led_fold != c.fold)
    return fail(CTCDEC_ERR_ARG, rs->led_fold ? "a stream keeps the confidence fold its first chunk asked for"
                                             : "token confidences have to be asked for from a stream's first chunk on");
  c.led = first ? c.fold : rs->led_fold;
  if (c.led && !first)
    for (int32_t u = 0; u < c.n_utts; ++u)
      if ((int64_t)c.stream->first_frame[u] != (int64_t)rs->led_first[(size_t)u] + rs->frames[(size_t)u])
        return fail(CTCDEC_ERR_ARG, "stream " + std::to_string(u) + ": first_frame " + std::to_string(c.stream->first_frame[u]) +
                                        " does not continue the stream (token confidences: expected " +
                                        std::to_string((int64_t)rs->led_first[(size_t)u] + rs->frames[(size_t)u]) + ")");
  return CTCDEC_OK;
}

// 1a. Argument checks; the (still empty) result.
static int check_call(DecodeCall& c) {
  const ctcdec_params* p = c.p;
  if (!c.dec || !p || !c.out || c.n_utts < 0 || (c.n_utts > 0 && (!c.utt_logits || !c.utt_frames)))
    return fail(CTCDEC_ERR_ARG, "bad arguments");
  if (c.dtype < CTCDEC_F32 || c.dtype > CTCDEC_BF16) return fail(CTCDEC_ERR_ARG, "dtype must be f32, f64, f16 or bf16");
  if (p->beam_width < 1) return fail(CTCDEC_ERR_ARG, "beam_width must be >= 1");
  if (p->beam_width > CTCDEC_MAX_BEAM_WIDTH)
    return fail(CTCDEC_ERR_LIMIT, "beam_width above the supported maximum of 256");
  c.fold = logp_fold(p);
  if (c.fold && c.stream && !c.rs)
    return fail(CTCDEC_ERR_ARG, "token confidences are not available to streaming decodes whose beams the caller hands in");
  if (c.rs)
    if (int rc = check_stream_tokens(c)) return rc;
  c.t_begin = Clock::now();
  c.res.reset(new ctcdec_result());
  c.res->utts.resize((size_t)c.n_utts);
  return CTCDEC_OK;
}

// 1b. The hand-over of armed hot-word sets, the device, the tables, the staging block, the row offsets.
static int open_call(DecodeCall& c) {
  ctcdec_decoder* dec = c.dec;
  const int32_t n_utts = c.n_utts;
  std::string& err = c.err;
  c.K = dec->has_lm ? dec->n_lms() : 1;
  if (dec->hot_call.armed) {
    if ((int32_t)dec->hot_call.utt_set.size() != n_utts) return fail(CTCDEC_ERR_ARG, "hot-word sets armed for another number of utterances");
    if (c.stream && !c.rs) build_hot_sets(dec->hot_call);  // (the imported beams' words are counted against their stream's set)
  }
  c.device_lock = std::unique_lock<std::mutex>(g_device_mu);
  if (be::bind_thread(&err)) return fail(CTCDEC_ERR_DEVICE, err);
  if (sync_tables(dec, &err)) return fail(CTCDEC_ERR_DEVICE, err);
  c.V = (int)dec->alpha.labels.size();
  c.B = c.p->beam_width;
  c.n_best = c.p->n_best > 0 ? std::min(c.p->n_best, c.B) : c.B;
  c.host_timing = getenv("CTCDEC_HOST_TIMING") != nullptr;
  // staging for this call's small uploads (every earlier call has synchronised: nothing is in flight from the block)
  dec->stage_used = 0;
  if (dec->h_stage.ensure((size_t)n_utts * (64 + sizeof(LmState) * (size_t)c.K) + 4096, &err)) return fail(CTCDEC_ERR_DEVICE, err);
  c.row0.assign((size_t)n_utts + 1, 0);
  for (int32_t u = 0; u < n_utts; ++u) {
    if (c.utt_frames[u] < 0) return fail(CTCDEC_ERR_ARG, "negative frame count");
    c.row0[(size_t)u + 1] = c.row0[(size_t)u] + c.utt_frames[u];
  }
  c.R = c.row0[(size_t)n_utts];
  return CTCDEC_OK;
}

// 2. Logits: device pointers are used in place, host matrices are staged.
static int stage_logits(DecodeCall& c) {
  ctcdec_decoder* dec = c.dec;
  std::string& err = c.err;
  const int32_t n_utts = c.n_utts;
  const size_t row_bytes = (size_t)c.V * dtype_size(c.dtype);
  c.ptrs.resize((size_t)n_utts);
  if (c.is_device) {
    for (int32_t u = 0; u < n_utts; ++u) c.ptrs[(size_t)u] = c.utt_logits[u];
  } else {
    if (dec->w_logits.ensure((size_t)std::max<int64_t>(c.R, 1) * row_bytes, &err)) return fail(CTCDEC_ERR_DEVICE, err);
    // (utterances that follow each other in host memory -- one [B, T, V] array -- go over in one copy)
    for (int32_t u = 0; u < n_utts;) {
      char* dst = (char*)dec->w_logits.p + (size_t)c.row0[(size_t)u] * row_bytes;
      const char* src = (const char*)c.utt_logits[u];
      size_t bytes = (size_t)c.utt_frames[u] * row_bytes;
      c.ptrs[(size_t)u] = dst;
      int32_t v = u + 1;
      while (v < n_utts && (const char*)c.utt_logits[v] == src + bytes) {
        c.ptrs[(size_t)v] = dst + bytes;
        bytes += (size_t)c.utt_frames[v] * row_bytes;
        ++v;
      }
      if (bytes && be::h2d(dst, src, bytes, &err)) return fail(CTCDEC_ERR_DEVICE, err);
      u = v;
    }
  }
  if (upload_staged(dec, dec->w_ptrs, c.ptrs, &err) || upload_staged(dec, dec->w_row0, c.row0, &err)) return fail(CTCDEC_ERR_DEVICE, err);
  return CTCDEC_OK;
}

// 3. Arenas of text nodes (one per completed-words prefix that is scored) and emission nodes (one per non-blank,
// non-repeat step of a kept beam). The worst case is beam_width of each per frame; what a frame really takes is a
// handful, so the usual reservation is 16 per frame (+ 2 beam_widths): an utterance that
// outgrows it reports ST_TEXT_OVERFLOW / ST_EMIT_OVERFLOW and the beam stage is redone with the worst case, which
// this decoder then keeps reserving. A resident stream's kernel cannot be redone: always the worst case (per chunk).
static void size_arenas(DecodeCall& c, bool full) {
  const uint64_t B = (uint64_t)c.B, K = (uint64_t)c.K;
  const uint64_t per_frame = full ? B : std::min<uint64_t>(B, 16);
  c.toff.assign((size_t)c.n_utts + 1, 0);
  c.eoff.assign((size_t)c.n_utts + 1, 0);
  for (int32_t u = 0; u < c.n_utts; ++u) {
    const uint64_t T = (uint64_t)c.utt_frames[u];
    const uint64_t n_imp = c.rs ? (uint64_t)c.rs->mirror[(size_t)u].n_carry
                                : c.stream ? (uint64_t)(c.stream->beam_off[u + 1] - c.stream->beam_off[u]) : 0;
    c.toff[(size_t)u + 1] = c.toff[(size_t)u] + ((T + 1) * per_frame + 2 * B + 2 + n_imp) * K;
    c.eoff[(size_t)u + 1] = c.eoff[(size_t)u] + T * per_frame + 2 * B + 2 + n_imp;
  }
}

// 4a. Resident streams: the chunk's first frames, and room for it in the streams' own emission arena (kept from their start).
static int stage_resident_input(DecodeCall& c) {
  ctcdec_stream* rs = c.rs;
  std::string& err = c.err;
  const int32_t n_utts = c.n_utts;
  for (int32_t u = 0; u < n_utts; ++u) c.ba.max_import = std::max<int32_t>(c.ba.max_import, (int32_t)rs->mirror[(size_t)u].n_carry);
  std::vector<int32_t> ff(c.stream->first_frame, c.stream->first_frame + n_utts);
  if (upload(c.dec->w_ff, ff, &err)) return fail(CTCDEC_ERR_DEVICE, err);
  uint64_t need = 0;
  for (int32_t u = 0; u < n_utts; ++u)
    need = std::max<uint64_t>(need, (uint64_t)rs->mirror[(size_t)u].emit_next + (uint64_t)c.utt_frames[u] * (uint64_t)c.B +
                                        (uint64_t)ctcdec_stream::CAP + 2);
  if (need <= rs->emit_cap) return CTCDEC_OK;
  // (sized for the worst case -- one node per frame and beam --, of which a real stream uses a few per cent: grow
  // in big steps so that a long stream reallocates a handful of times)
  const uint64_t cap = std::max<uint64_t>(std::max<uint64_t>(4 * need, 2 * rs->emit_cap), 4096);
  DevBuf grown;  // (a failure below releases it: the stream keeps its old arena)
  if (grown.ensure((size_t)n_utts * cap * sizeof(EmitNode), &err)) return fail(CTCDEC_ERR_DEVICE, err);
  for (int32_t u = 0; u < n_utts && rs->emit.p; ++u) {
    const size_t used = (size_t)rs->mirror[(size_t)u].emit_next * sizeof(EmitNode);
    if (used && be::d2d((char*)grown.p + (size_t)u * cap * sizeof(EmitNode), (const char*)rs->emit.p + (size_t)u * rs->emit_cap * sizeof(EmitNode), used, &err))
      return fail(CTCDEC_ERR_DEVICE, err);
  }
  // the new offsets first: a failure here leaves the stream on its old arena with its old stride
  std::vector<uint64_t> eo((size_t)n_utts + 1);
  for (int32_t u = 0; u <= n_utts; ++u) eo[(size_t)u] = (uint64_t)u * cap;
  if (upload(rs->eoff, eo, &err)) return fail(CTCDEC_ERR_DEVICE, err);
  rs->emit = std::move(grown);
  rs->emit_cap = cap;
  return CTCDEC_OK;
}

// 4b. Streams whose beams the caller hands in: every stream's carried-over beams, resolved on the host (build_import).
static int stage_imports(DecodeCall& c) {
  ctcdec_decoder* dec = c.dec;
  const StreamIn* stream = c.stream;
  std::string& err = c.err;
  const int32_t n_utts = c.n_utts;
  const int K = c.K;
  const int64_t n_imp_total = stream->beam_off[n_utts];
  std::vector<ImportBeam> imps((size_t)std::max<int64_t>(n_imp_total, 1));
  std::vector<LmState> imps_x(K > 1 ? (size_t)std::max<int64_t>(n_imp_total, 1) * (size_t)(K - 1) : 0);
  std::vector<int64_t> ioff(stream->beam_off, stream->beam_off + n_utts + 1);
  std::vector<int32_t> ff(stream->first_frame, stream->first_frame + n_utts);
  for (int32_t u = 0; u < n_utts; ++u) {
    int64_t cnt = ioff[(size_t)u + 1] - ioff[(size_t)u];
    if (cnt < 1 || cnt > beam_bucket(c.B))
      return fail(CTCDEC_ERR_ARG, "a stream must carry between 1 and beam-capacity beams");
    c.ba.max_import = std::max<int32_t>(c.ba.max_import, (int32_t)cnt);
    for (int64_t k = ioff[(size_t)u]; k < ioff[(size_t)u + 1]; ++k) {
      std::string e = build_import(dec, *stream, k, &imps[(size_t)k], K > 1 ? &imps_x[(size_t)k * (size_t)(K - 1)] : nullptr,
                                   import_hot(dec, u));
      if (!e.empty()) return fail(CTCDEC_ERR_ARG, e);
    }
  }
  if (upload(dec->w_imp, imps, &err) || upload(dec->w_impoff, ioff, &err) || upload(dec->w_ff, ff, &err))
    return fail(CTCDEC_ERR_DEVICE, err);
  if (K > 1 && upload(dec->w_impx, imps_x, &err)) return fail(CTCDEC_ERR_DEVICE, err);
  return CTCDEC_OK;
}

// The arenas, the output records and the emission-list pool of the beam stage.
static int reserve_beam_workspace(DecodeCall& c) {
  ctcdec_decoder* dec = c.dec;
  std::string& err = c.err;
  const int32_t n_utts = c.n_utts;
  // emission lists: at most one entry per frame plus the import root and the closing entry
  c.tok_cap = (unsigned long long)c.n_best * (unsigned long long)(c.R + 2 * (int64_t)n_utts);
  if (c.rs) {
    // A resident stream's lists reach back to its start, but a beam's chain holds at most one entry per frame pushed so
    // far, one per chunk (a word closed by force_next_word) and its root -- NOT the stream's whole emission arena (every
    // beam's nodes: ten minutes of audio on 64 streams would ask for gigabytes here; round-3 advisor finding).
    unsigned long long depth = 0;
    for (int32_t u = 0; u < n_utts; ++u)
      depth += (unsigned long long)(c.rs->frames[(size_t)u] + c.utt_frames[u] + c.rs->pushes + 3);
    c.tok_cap = c.want_result ? (unsigned long long)c.n_best * depth : 1ull;
  }
  if (dec->w_text.ensure(c.toff[(size_t)n_utts] * sizeof(TextNode), &err) ||
      (!c.rs && (dec->w_emit.ensure(c.eoff[(size_t)n_utts] * sizeof(EmitNode), &err) || upload_staged(dec, dec->w_eoff, c.eoff, &err))) ||
      upload_staged(dec, dec->w_toff, c.toff, &err) || dec->w_out.ensure((size_t)n_utts * c.n_best * sizeof(OutBeam), &err) ||
      dec->w_nout.ensure((size_t)n_utts * 4, &err) || dec->w_status.ensure((size_t)n_utts * 4, &err) ||
      dec->w_tok.ensure((size_t)std::max<unsigned long long>(c.tok_cap, 1) * sizeof(EmitNode), &err) ||
      dec->w_head.ensure(16, &err) || dec->w_cold.ensure((size_t)n_utts * 2 * COLD_STRIDE * sizeof(ColdRec), &err))
    return fail(CTCDEC_ERR_DEVICE, err);
  return CTCDEC_OK;
}

// 5. Start states: per utterance one state per model; a negative length (or no array) asks for the model's own default.
// (Host imports: none, every beam carries its own. Resident streams: used by the streams that are at their starting state.)
static int stage_start_states(DecodeCall& c) {
  ctcdec_decoder* dec = c.dec;
  const int K = c.K;
  c.xstate_bytes = K > 1 ? (size_t)c.n_utts * c.n_best * (size_t)(K - 1) * sizeof(LmState) : 0;
  if (!(c.stream && !c.rs) && dec->has_lm) {
    std::vector<LmState> st((size_t)c.n_utts * K);
    for (int32_t u = 0; u < c.n_utts; ++u) {
      for (int k = 0; k < K; ++k) {
        LmState& s = st[(size_t)u * K + k];
        const HostLM& lm = K > 1 ? *dec->multi->lms[(size_t)k] : dec->lm_ref();
        const ctcdec_lm_state* given = c.start_states ? &c.start_states[(size_t)u * K + k] : nullptr;
        if (!given || given->length < 0) {
          const bool boundary = k == 0 ? c.p->lm_score_boundary != 0 : dec->x_boundary[k] != 0;
          memset(&s, 0, sizeof(s));
          lm.start_state(boundary, &s);
        } else if (const LmStateErr e = copy_lm_state(*given, lm.words.size(), &s)) {
          return fail(CTCDEC_ERR_ARG, e == LM_STATE_LENGTH ? "LM start state too long" : "bad LM state word");
        }
      }
    }
    if (upload_staged(dec, dec->w_start, st, &c.err)) return fail(CTCDEC_ERR_DEVICE, c.err);
    c.ba.start_states = (const LmState*)dec->w_start.p;
  }
  if (c.xstate_bytes && dec->w_xstate.ensure(c.xstate_bytes, &c.err)) return fail(CTCDEC_ERR_DEVICE, c.err);
  return CTCDEC_OK;
}

// device texts: scratch per utterance -- at most one emission per frame, each a label and a separator
static int reserve_device_texts(DecodeCall& c) {
  ctcdec_decoder* dec = c.dec;
  std::vector<uint64_t> soff((size_t)c.n_utts + 1, 0);
  for (int32_t u = 0; u < c.n_utts; ++u)
    soff[(size_t)u + 1] = soff[(size_t)u] + (((uint64_t)c.utt_frames[u] + 2) * (uint64_t)(dec->max_label_bytes + 1) + 15) / 16 * 16;
  if (dec->w_tscr.ensure((size_t)soff[(size_t)c.n_utts] + 16, &c.err) || dec->w_tpool.ensure((size_t)soff[(size_t)c.n_utts] + 16, &c.err) ||
      upload_staged(dec, dec->w_tsoff, soff, &c.err))
    return fail(CTCDEC_ERR_DEVICE, c.err);
  c.ba.text_scratch = (uint8_t*)dec->w_tscr.p;
  c.ba.text_soff = (const uint64_t*)dec->w_tsoff.p;
  c.ba.text_pool = (uint8_t*)dec->w_tpool.p;
  c.ba.text_pool_cap = soff[(size_t)c.n_utts];
  return CTCDEC_OK;
}

// ragged batches of more utterances than fit the device at once: longest first (BeamArgs::order)
static int stage_longest_first(DecodeCall& c) {
  const int32_t* utt_frames = c.utt_frames;
  if (c.n_utts <= be::cus() * 2 || getenv("CTCDEC_NO_LPT_ORDER")) return CTCDEC_OK;
  bool ragged = false;
  for (int32_t u = 1; u < c.n_utts; ++u) ragged = ragged || utt_frames[u] != utt_frames[0];
  if (!ragged) return CTCDEC_OK;
  std::vector<int32_t> order((size_t)c.n_utts);
  for (int32_t u = 0; u < c.n_utts; ++u) order[(size_t)u] = u;
  std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return utt_frames[x] > utt_frames[y]; });
  if (upload(c.dec->w_order, order, &c.err)) return fail(CTCDEC_ERR_DEVICE, c.err);
  c.ba.order = (const int32_t*)c.dec->w_order.p;
  return CTCDEC_OK;
}

// 6. The beam stage's arguments (the survivor lists and the wave kernel's payload follow per prune attempt: beam_ready).
static int fill_beam_args(DecodeCall& c) {
  ctcdec_decoder* dec = c.dec;
  const ctcdec_params* p = c.p;
  const StreamIn* stream = c.stream;
  ctcdec_stream* rs = c.rs;
  be::BeamArgs& ba = c.ba;
  device_tables(dec, &ba.tables);
  DecodeParams& dp = ba.params;
  memset(&dp, 0, sizeof(dp));
  dp.beam_width = c.B;
  dp.prune_history = p->prune_history ? 1 : 0;
  dp.n_best = c.n_best;
  dp.first_frame = p->first_frame;
  dp.beam_prune_logp = p->beam_prune_logp;
  dp.token_min_logp = p->token_min_logp;
  dp.hot_weight = p->hotword_weight;
  dp.alpha = p->alpha;
  dp.beta = p->beta;
  dp.unk = p->unk_score_offset;
  dp.log_base_change = p->log_base_change;
  dp.score_boundary = p->lm_score_boundary ? 1 : 0;
  dp.fold = stream ? stream->fold : 1;
  dp.eos = stream ? stream->eos : 1;
  dp.no_label_runs = getenv("CTCDEC_NO_LABEL_RUNS") != nullptr ? 1 : 0;
  // decode_batch: the kernels assemble the best beam's text themselves (CTCDEC_HOST_REPLAY=1: the emission lists come
  // back and the host replays them, as for every other call)
  c.device_texts = p->texts_only != 0 && p->token_frames == 0 && c.n_best == 1 && !stream && getenv("CTCDEC_HOST_REPLAY") == nullptr;
  dp.texts_only = c.device_texts ? 1 : 0;
  ba.n_utts = c.n_utts;
  ba.utt_row0 = (const int64_t*)dec->w_row0.p;
  ba.text_nodes = (TextNode*)dec->w_text.p;
  ba.text_off = (const uint64_t*)dec->w_toff.p;
  ba.out_xstates = c.xstate_bytes ? (LmState*)dec->w_xstate.p : nullptr;
  ba.out = (OutBeam*)dec->w_out.p;
  ba.out_stride = c.n_best;
  ba.n_out = (uint32_t*)dec->w_nout.p;
  ba.status = (uint32_t*)dec->w_status.p;
  ba.tok_pool = (EmitNode*)dec->w_tok.p;
  ba.tok_pool_head = (unsigned long long*)dec->w_head.p;
  ba.tok_pool_cap = c.tok_cap;
  ba.first_frames = stream ? (const int32_t*)dec->w_ff.p : nullptr;
  ba.cold = (ColdRec*)dec->w_cold.p;
  ba.want_out = 1;
  ba.total_rows = c.R;
  if (c.device_texts)
    if (int rc = reserve_device_texts(c)) return rc;
  if (int rc = stage_longest_first(c)) return rc;
  // where the emission nodes go and where the carried-over beams come from
  if (rs) {
    ba.emit_nodes = (EmitNode*)rs->emit.p;
    ba.emit_off = (const uint64_t*)rs->eoff.p;
    ba.imports = (const ImportBeam*)rs->carry.p;
    ba.import_xstates = c.K > 1 ? (const LmState*)rs->carry_x.p : nullptr;
    ba.resident_in = 1;
    ba.carry_out = (ImportBeam*)rs->carry.p;
    ba.carry_xstates = c.K > 1 ? (LmState*)rs->carry_x.p : nullptr;
    ba.sstate = (StreamState*)rs->sstate.p;
    ba.carry_stride = ctcdec_stream::CAP;
    ba.want_out = c.want_result ? 1 : 0;
  } else {
    ba.emit_nodes = (EmitNode*)dec->w_emit.p;
    ba.emit_off = (const uint64_t*)dec->w_eoff.p;
    if (stream) {
      ba.imports = (const ImportBeam*)dec->w_imp.p;
      ba.import_xstates = c.K > 1 ? (const LmState*)dec->w_impx.p : nullptr;
      ba.import_off = (const int64_t*)dec->w_impoff.p;
    }
  }
  if (dec->profile) {
    if (dec->w_prof.ensure(N_PROF * 8, &c.err) || be::zero(dec->w_prof.p, N_PROF * 8, &c.err)) return fail(CTCDEC_ERR_DEVICE, c.err);
    ba.prof = (unsigned long long*)dec->w_prof.p;
  }
  if (dec->w_flags.ensure(32, &c.err) || dec->w_head.ensure(16, &c.err)) return fail(CTCDEC_ERR_DEVICE, c.err);
  // Small batches choose their beam kernel by the input (backend: wave_kernel_chosen): their beam stage is launched when the
  // prune stage has reported -- like a resident stream's --, one small read-back between the two stages.
  c.by_input = !rs && be::beam_kernel_depends_on_input(ba);
  c.late_beam = rs != nullptr || c.by_input;
  return CTCDEC_OK;
}

// the wave kernel's payload lines (one per candidate a frame can push into its pool)
static int reserve_pay(DecodeCall& c) {
  be::BeamArgs& ba = c.ba;
  ba.pay = nullptr;
  ba.pay_stride = 0;
  if (be::wave_kernel_chosen(ba)) {  // reserved only for launches that will use it (2 GB at the bench size)
    ba.pay_stride = (uint64_t)wave_pay_stride(ba.params);
    if (c.dec->w_pay.ensure((size_t)c.n_utts * (size_t)ba.pay_stride * sizeof(PoolPay), &c.err)) return fail(CTCDEC_ERR_DEVICE, c.err);
    ba.pay = (PoolPay*)c.dec->w_pay.p;
  }
  return CTCDEC_OK;
}

static int run_beam(DecodeCall& c) {
  if (be::zero(c.dec->w_head.p, 16, &c.err)) return fail(CTCDEC_ERR_DEVICE, c.err);
  // per-utterance hot words: built and sent here, behind the first prune launch -- the host builds the tables while the
  // prune stage runs
  if (c.dec->hot_call.armed && !c.ba.hot_sets && upload_hot_sets(c.dec, &c.ba, &c.err)) return fail(CTCDEC_ERR_DEVICE, c.err);
  if (be::launch_beam(c.ba, &c.err)) return fail(CTCDEC_ERR_DEVICE, c.err);
  return CTCDEC_OK;
}

// A prune attempt's survivor lists are reserved, max_surv wide: the beam stage reads them (and sizes its payload by them).
static int beam_ready(DecodeCall& c, int max_surv) {
  c.ba.surv_cnt = (const uint32_t*)c.dec->w_scnt.p;
  c.ba.surv_id = (const uint16_t*)c.dec->w_sid.p;
  c.ba.surv_lp = (const double*)c.dec->w_slp.p;
  c.ba.params.max_surv = max_surv;
  return c.by_input ? CTCDEC_OK : reserve_pay(c);
}

// survivor bound: rows are normalised log-probabilities, so at most floor(e^-min) labels pass
static int max_surv_bound(double token_min_logp, int V) {
  int max_surv = V;
  if (token_min_logp > log(1e-15)) {  // frames are clipped at ln(MIN_TOKEN_CLIP_P) (constants.py:17)
    double bound = floor(exp(-token_min_logp)) + 2.0;
    if (bound < (double)V) max_surv = (int)bound;
  }
  return max_surv < 1 ? 1 : max_surv;
}

// The frame-prune stage: pass 0 (every utterance as logits), the exact probability test for the utterances pass 0 marked
// ambiguous, pass 1 for the probability-like ones, and -- un-normalised probability rows can exceed the survivor bound -- all
// of it again at full width. `beam`: the decode whose beam stage reads the lists, or nullptr (ctcdec_frame_survivors).
// Everything the beam stage needs is staged BEFORE the prune launch and the beam kernel is queued right behind it on the same
// stream: the host never sits between the two kernels. The two rare events (probability-like input, survivor overflow) are read
// back afterwards and simply redo the affected stage(s). (late_beam -- resident streams, whose kernel advances persistent state,
// and small batches, whose kernel is chosen by what the prune stage counted -- launch it once the stage has reported.)
int prune_stage(PruneStage& s, DecodeCall* beam) {
  ctcdec_decoder* dec = s.dec;
  std::string err;
  const int V = s.V;
  const size_t rows = (size_t)std::max<int64_t>(s.R, 1);
  uint32_t* flags = s.flags;
  s.max_surv = max_surv_bound(s.token_min_logp, V);
  for (int attempt = 0;; ++attempt) {
    const size_t max_surv = (size_t)s.max_surv;
    if (dec->w_rowsum.ensure(rows * 8, &err) || dec->w_isprob.ensure((size_t)s.n_utts * 4, &err) ||
        dec->w_scnt.ensure(rows * 4, &err) || dec->w_sid.ensure(rows * max_surv * 2, &err) ||
        dec->w_slp.ensure(rows * max_surv * 8, &err) || dec->w_flags.ensure(32, &err) || dec->w_slow.ensure(rows * 4, &err))
      return fail(CTCDEC_ERR_DEVICE, err);
    if (be::zero(dec->w_flags.p, 32, &err)) return fail(CTCDEC_ERR_DEVICE, err);
    be::PruneArgs pa;
    pa.utt_logits = (const void* const*)dec->w_ptrs.p;
    pa.utt_row0 = (const int64_t*)dec->w_row0.p;
    pa.n_utts = s.n_utts;
    pa.n_rows = s.R;
    pa.n_labels = V;
    pa.dtype = s.dtype;
    pa.token_min_logp = s.token_min_logp;
    pa.max_surv = s.max_surv;
    pa.row_sum = (double*)dec->w_rowsum.p;
    pa.utt_is_prob = (uint32_t*)dec->w_isprob.p;
    pa.surv_cnt = (uint32_t*)dec->w_scnt.p;
    pa.surv_id = (uint16_t*)dec->w_sid.p;
    pa.surv_lp = (double*)dec->w_slp.p;
    pa.overflow = (uint32_t*)dec->w_flags.p;
    pa.pass = 0;
    pa.row_base = 0;
    pa.slow_rows = (uint32_t*)dec->w_slow.p;
    const bool sliced = beam && dec->slicing;  // (time-sliced host ingest: each slice's side of 1 is noted for decode_host_sliced)
    pa.utt_side = sliced ? (uint32_t*)dec->w_side.p : nullptr;
    pa.utt_sum = sliced ? (double*)((char*)dec->w_side.p + (((size_t)s.n_utts * 4 + 15) & ~(size_t)15)) : nullptr;
    pa.dense_hint = 0;
    if (beam && dec->dense_calls > 0 && !s.resident) {
      pa.dense_hint = 1;
      if (attempt == 0) --dec->dense_calls;
    }
    pa.rows_aligned16 = 1;
    pa.rows_aligned4 = 1;
    for (const void* q : *s.ptrs) {
      if (((uintptr_t)q & 15u) != 0) pa.rows_aligned16 = 0;
      if (((uintptr_t)q & 3u) != 0) pa.rows_aligned4 = 0;
    }
    if (beam)
      if (int rc = beam_ready(*beam, s.max_surv)) return rc;
    const bool early_beam = beam && !beam->late_beam;
    s.t_setup = Clock::now();
    if (be::launch_prune(pa, &err)) return fail(CTCDEC_ERR_DEVICE, err);
    if (early_beam)
      if (int rc = run_beam(*beam)) return rc;
    s.t_queued = Clock::now();
    if (be::d2h(flags, dec->w_flags.p, 32, &err)) return fail(CTCDEC_ERR_DEVICE, err);
    s.t_flags = Clock::now();
    s.surv_total = flags[4];  // (pass 0 counted every row as logits)
    // small vocabularies fed flat logits: nearly every row overflows the 64-rows-per-wave kernel's sixteen candidates and is done
    // again by the per-row kernel -- the next sixteen calls go there directly (then the fast kernel is tried again)
    if (beam && V <= 128 && s.R >= 1024 && (uint64_t)flags[3] * 2 > (uint64_t)s.R) dec->dense_calls = 16;
    if (flags[2]) {  // rows that sum to about 1: the reference's test in its own dtype and summation order (decoder.py:760)
      if (be::launch_sniff_exact(pa, &err) || be::d2h(flags, dec->w_flags.p, 16, &err)) return fail(CTCDEC_ERR_DEVICE, err);
    }
    if (flags[1]) {  // some utterance holds probabilities: redo those rows as log(clip(p)), then the beams
      pa.pass = 1;
      // pass-0 overflows of those rows are void, and so is its survivor count (flags[4]: the pass counts them again)
      if (be::zero(dec->w_flags.p, 4, &err) || be::zero((char*)dec->w_flags.p + 16, 4, &err)) return fail(CTCDEC_ERR_DEVICE, err);
      if (be::launch_prune(pa, &err)) return fail(CTCDEC_ERR_DEVICE, err);
      if (early_beam)
        if (int rc = run_beam(*beam)) return rc;
      if (be::d2h(flags, dec->w_flags.p, 32, &err)) return fail(CTCDEC_ERR_DEVICE, err);
      s.surv_total = flags[4];
    }
    if (!flags[0]) return CTCDEC_OK;
    if (s.max_surv == V) return fail(CTCDEC_ERR_INTERNAL, "survivor overflow at full vocabulary");
    s.max_surv = V;  // un-normalised probability rows can exceed the bound: redo at full width
  }
}

// Resident streams with a survivor ledger: room for this chunk. The host knows the entries each stream held after the last push
// exactly and this chunk's worst case (frames x the width the prune stage ended with); like the emission arena the ledger
// grows in big steps with a device-to-device copy of the used part, and a failure leaves the stream on its old ledger.
static int reserve_ledger(DecodeCall& c) {
  ctcdec_stream* rs = c.rs;
  std::string& err = c.err;
  const int32_t n = c.n_utts;
  const bool first = rs->pushes == 0;
  if (first) {
    rs->led_used.assign((size_t)n, 0);
    rs->led_first.assign(c.stream->first_frame, c.stream->first_frame + n);
  }
  uint64_t need_rows = 0, need_ent = 0;
  for (int32_t u = 0; u < n; ++u) {
    const uint64_t chunk = (uint64_t)c.utt_frames[u] * (uint64_t)c.prune.max_surv;
    if (chunk > UINT32_MAX || (uint64_t)rs->frames[(size_t)u] + (uint64_t)c.utt_frames[u] > UINT32_MAX)
      return fail(CTCDEC_ERR_LIMIT, "token confidences: a chunk of more than 2^32 survivor entries, or a stream of more than 2^32 frames");
    need_rows = std::max<uint64_t>(need_rows, (uint64_t)rs->frames[(size_t)u] + (uint64_t)c.utt_frames[u]);
    need_ent = std::max<uint64_t>(need_ent, rs->led_used[(size_t)u] + chunk);
  }
  if (need_rows > rs->led_row_cap || need_ent > rs->led_ent_cap || !rs->led_off.p) {
    const uint64_t row_cap = std::max<uint64_t>(std::max<uint64_t>(2 * need_rows, 2 * rs->led_row_cap), 1024);
    const uint64_t ent_cap = std::max<uint64_t>(std::max<uint64_t>(2 * need_ent, 2 * rs->led_ent_cap), 4096);
    DevBuf off, id, lp;  // (a failure below releases them: the stream keeps its old ledger)
    if (off.ensure((size_t)n * (row_cap + 1) * 8, &err) || id.ensure((size_t)n * ent_cap * 2, &err) || lp.ensure((size_t)n * ent_cap * 8, &err))
      return fail(CTCDEC_ERR_DEVICE, err);
    for (int32_t u = 0; u < n && rs->led_off.p && !first; ++u) {
      const size_t rows = (size_t)rs->frames[(size_t)u], used = (size_t)rs->led_used[(size_t)u];
      if (be::d2d((char*)off.p + (size_t)u * (row_cap + 1) * 8, (const char*)rs->led_off.p + (size_t)u * (rs->led_row_cap + 1) * 8, (rows + 1) * 8, &err) ||
          (used && (be::d2d((char*)id.p + (size_t)u * ent_cap * 2, (const char*)rs->led_id.p + (size_t)u * rs->led_ent_cap * 2, used * 2, &err) ||
                    be::d2d((char*)lp.p + (size_t)u * ent_cap * 8, (const char*)rs->led_lp.p + (size_t)u * rs->led_ent_cap * 8, used * 8, &err))))
        return fail(CTCDEC_ERR_DEVICE, err);
    }
    rs->led_off = std::move(off);
    rs->led_id = std::move(id);
    rs->led_lp = std::move(lp);
    rs->led_row_cap = row_cap;
    rs->led_ent_cap = ent_cap;
  }
  if (first && be::zero((char*)rs->sstate.p + rs->sstate_bytes(), (size_t)n * 8 + 8, &err)) return fail(CTCDEC_ERR_DEVICE, err);
  rs->led_fold = c.led;
  return CTCDEC_OK;
}

// ... and the chunk's rows into it: once per push, behind the beam kernel on the decode stream.
static int append_ledger(DecodeCall& c) {
  ctcdec_stream* rs = c.rs;
  ctcdec_decoder* dec = c.dec;
  const int32_t n = c.n_utts;
  const uint32_t max_surv = (uint32_t)c.prune.max_surv;
#ifdef CTC_SIM  // (the simulator's device memory is host memory: the kernel's body, row by row)
  const uint32_t* cnt = (const uint32_t*)dec->w_scnt.p;
  const uint16_t* sid = (const uint16_t*)dec->w_sid.p;
  const double* slp = (const double*)dec->w_slp.p;
  uint64_t* used_out = (uint64_t*)((char*)rs->sstate.p + rs->sstate_bytes());
  for (int32_t u = 0; u < n; ++u) {
    uint64_t* ro = (uint64_t*)rs->led_off.p + (size_t)u * (rs->led_row_cap + 1);
    uint16_t* did = (uint16_t*)rs->led_id.p + (size_t)u * rs->led_ent_cap;
    double* dlp = (double*)rs->led_lp.p + (size_t)u * rs->led_ent_cap;
    const size_t r0 = (size_t)rs->frames[(size_t)u];
    if (r0 == 0) ro[0] = 0;
    uint64_t base = ro[r0];
    for (int32_t t = 0; t < c.utt_frames[u]; ++t) {
      const size_t src = (size_t)c.row0[(size_t)u] + (size_t)t;
      const uint32_t k = ledger_row_count(cnt[src], max_surv);
      if (base + k > rs->led_ent_cap || r0 + (size_t)t + 1 > rs->led_row_cap) {
        used_out[n] = 1;
        break;
      }
      ledger_put_row(sid + src * max_surv, slp + src * max_surv, k, did + base, dlp + base);
      base += k;
      ro[r0 + (size_t)t + 1] = base;
    }
    used_out[u] = base;
  }
#else
  std::vector<uint32_t> r0((size_t)n);
  for (int32_t u = 0; u < n; ++u) r0[(size_t)u] = (uint32_t)rs->frames[(size_t)u];
  if (upload_staged(dec, dec->w_ledrow, r0, &c.err)) return fail(CTCDEC_ERR_DEVICE, c.err);
  be::LedgerAppendArgs la;
  la.n_streams = n;
  la.utt_row0 = (const int64_t*)dec->w_row0.p;
  la.surv_cnt = (const uint32_t*)dec->w_scnt.p;
  la.surv_id = (const uint16_t*)dec->w_sid.p;
  la.surv_lp = (const double*)dec->w_slp.p;
  la.max_surv = (int32_t)max_surv;
  la.led_row0 = (const uint32_t*)dec->w_ledrow.p;
  la.row_off = (uint64_t*)rs->led_off.p;
  la.id = (uint16_t*)rs->led_id.p;
  la.lp = (double*)rs->led_lp.p;
  la.row_cap = rs->led_row_cap;
  la.ent_cap = rs->led_ent_cap;
  la.used_out = (uint64_t*)((char*)rs->sstate.p + rs->sstate_bytes());
  la.overrun = la.used_out + n;
  if (be::launch_ledger_append(la, &c.err)) return fail(CTCDEC_ERR_DEVICE, c.err);
#endif
  return CTCDEC_OK;
}

// 7. Prune and launch: the prune stage with the beam stage queued right behind it, or -- late_beam -- once it has reported.
static int prune_and_launch(DecodeCall& c) {
  PruneStage& s = c.prune;
  s = PruneStage{c.dec, &c.ptrs, c.n_utts, c.dtype, c.R, c.V, c.p->token_min_logp, c.rs != nullptr};
  s.t_setup = s.t_queued = s.t_flags = c.t_begin;
  if (int rc = prune_stage(s, &c)) return rc;
  if (c.by_input) {
    const double mean = c.R > 0 ? (double)s.surv_total / (double)c.R : 0.0;
    c.ba.surv_x16 = (int32_t)std::min(1.0e6, std::max(1.0, mean * 16.0 + 0.5));
    if (int rc = reserve_pay(c)) return rc;
  }
  // (a stream with a ledger: room for the chunk first -- a failed growth leaves the stream where it was --, the append behind
  // the beam kernel. The lists are final here: every redo of the prune stage is over.)
  if (c.led)
    if (int rc = reserve_ledger(c)) return rc;
  if (c.late_beam)
    if (int rc = run_beam(c)) return rc;
  return c.led && c.R > 0 ? append_ledger(c) : CTCDEC_OK;  // (a read pushes no rows)
}

// (rare: flat posteriors that complete a word for every beam in every frame) the beam stage again, with the worst case reserved
static int redo_outgrown(DecodeCall& c) {
  ctcdec_decoder* dec = c.dec;
  std::string& err = c.err;
  const int32_t n_utts = c.n_utts;
  if (getenv("CTCDEC_ARENA_TRACE")) fprintf(stderr, "[ctcdec host] node arenas outgrown: beam stage redone with the worst case\n");
  dec->arenas_worst_case = true;
  c.arenas_full = true;
  c.outgrown_redone = true;
  size_arenas(c, true);
  if (dec->w_text.ensure(c.toff[(size_t)n_utts] * sizeof(TextNode), &err) ||
      dec->w_emit.ensure(c.eoff[(size_t)n_utts] * sizeof(EmitNode), &err) || upload(dec->w_toff, c.toff, &err) ||
      upload(dec->w_eoff, c.eoff, &err))
    return fail(CTCDEC_ERR_DEVICE, err);
  c.ba.text_nodes = (TextNode*)dec->w_text.p;
  c.ba.emit_nodes = (EmitNode*)dec->w_emit.p;
  c.ba.text_off = (const uint64_t*)dec->w_toff.p;
  c.ba.emit_off = (const uint64_t*)dec->w_eoff.p;
  if (be::zero(dec->w_head.p, 16, &err) || be::launch_beam(c.ba, &err) ||
      be::d2h(c.n_out, dec->w_nout.p, (size_t)n_utts * 4, &err) || be::d2h(c.status, dec->w_status.p, (size_t)n_utts * 4, &err) ||
      be::d2h(&c.head, dec->w_head.p, 8, &err))
    return fail(CTCDEC_ERR_DEVICE, err);
  return CTCDEC_OK;
}

// the streams have moved on, whatever the chunk's outcome: the host mirrors of their counters
static int refresh_stream_mirrors(DecodeCall& c) {
  ctcdec_stream* rs = c.rs;
  const size_t n = (size_t)c.n_utts;
  bool overrun = false;
  if (c.led) {  // (the ledger's entry counts ride behind the counters: one read for both)
    rs->led_back.resize(2 * n + n + 1);
    if (be::d2h(rs->led_back.data(), rs->sstate.p, rs->sstate_bytes() + n * 8 + 8, &c.err)) return fail(CTCDEC_ERR_DEVICE, c.err);
    memcpy(rs->mirror.data(), rs->led_back.data(), rs->sstate_bytes());
    for (size_t u = 0; u < n; ++u) rs->led_used[u] = rs->led_back[2 * n + u];
    overrun = rs->led_back[3 * n] != 0;
  } else if (be::d2h(rs->mirror.data(), rs->sstate.p, rs->sstate_bytes(), &c.err)) {
    return fail(CTCDEC_ERR_DEVICE, c.err);
  }
  for (int32_t u = 0; u < c.n_utts; ++u) rs->frames[(size_t)u] += c.utt_frames[u];
  rs->pushes += 1;
  if (c.led) c.led_rows.assign(rs->frames.begin(), rs->frames.end());
  if (c.stream->eos) {  // decoder.py:681-728 with is_end: the next chunk starts a new utterance
    for (auto& m : rs->mirror) {
      m.n_carry = 0;
      m.emit_next = 1;
      m.status = 0;
    }
    if (be::h2d(rs->sstate.p, rs->mirror.data(), (size_t)c.n_utts * sizeof(StreamState), &c.err)) return fail(CTCDEC_ERR_DEVICE, c.err);
    rs->has_import = false;
    std::fill(rs->frames.begin(), rs->frames.end(), 0);
    rs->pushes = 0;
    rs->led_fold = 0;  // (the next utterance chooses anew; this call's own fold still reads the rows: c.led_rows)
  }
  if (overrun) return fail(CTCDEC_ERR_INTERNAL, "survivor ledger: a chunk ran past the room reserved for it");
  return CTCDEC_OK;
}

// 8. The beam stage's counters back (page-locked staging), the outgrown-arena redo, the streams' mirrors, the refusals.
static int collect_counters(DecodeCall& c) {
  ctcdec_decoder* dec = c.dec;
  std::string& err = c.err;
  const int32_t n_utts = c.n_utts;
  c.t_launch = Clock::now();
  if (dec->h_small.ensure((size_t)n_utts * 8 + 16, &err) ||
      dec->h_out.ensure((size_t)n_utts * c.n_best * sizeof(OutBeam), &err))
    return fail(CTCDEC_ERR_DEVICE, err);
  c.n_out = (uint32_t*)dec->h_small.p;
  c.status = c.n_out + n_utts;
  // (one wait for the three: the targets are page-locked, `heads` rides in the spare 16 bytes behind the status words)
  c.heads_pinned = (unsigned long long*)(c.status + n_utts);
  if (be::d2h_async(c.n_out, dec->w_nout.p, (size_t)n_utts * 4, &err) ||
      be::d2h_async(c.status, dec->w_status.p, (size_t)n_utts * 4, &err) || be::d2h_async(c.heads_pinned, dec->w_head.p, 16, &err) ||
      be::sync(&err))
    return fail(CTCDEC_ERR_DEVICE, err);
  c.head = c.heads_pinned[0];
  if (!c.arenas_full) {
    bool outgrown = false;
    for (int32_t u = 0; u < n_utts; ++u) outgrown = outgrown || (c.status[u] & (ST_TEXT_OVERFLOW | ST_EMIT_OVERFLOW)) != 0;
    if (outgrown)
      if (int rc = redo_outgrown(c)) return rc;
  }
  c.t_kernel = Clock::now();
  if (c.rs)
    if (int rc = refresh_stream_mirrors(c)) return rc;
  for (int32_t u = 0; u < n_utts; ++u)
    if (c.status[u] & ST_NO_BEAMS)  // the reference: ValueError from max([]) (decoder.py:545 / :585)
      return fail(CTCDEC_ERR_ARG, "max() arg is an empty sequence (utterance " + std::to_string(u) +
                                      ": no beam survived -- non-finite scores or a positive beam_prune_logp)");
  for (int32_t u = 0; u < n_utts; ++u)
    if (c.status[u]) return fail(CTCDEC_ERR_INTERNAL, "beam kernel status " + std::to_string(c.status[u]) +
                                                          " for utterance " + std::to_string(u));
  return CTCDEC_OK;
}

// The closing step of every result form. When the beam stage's output is back: the kernels' times, the profile counters ...
static int kernel_stats(DecodeCall& c) {
  ctcdec_result* res = c.res.get();
#ifndef CTC_SIM
  if (c.led && c.R > 0 && c.host_timing)
    fprintf(stderr, "[ctcdec host] survivor ledger: surv_ledger_append kernel %.4f ms, %zu bytes reserved\n", be::last_ledger_append_ms(),
            c.rs->led_bytes());
#endif
  be::last_timing(&res->ms[0], &res->ms[1]);
  res->beam_kernel = be::last_beam_kernel();
  if (c.dec->profile && be::d2h(c.dec->prof, c.dec->w_prof.p, N_PROF * 8, &c.err)) return fail(CTCDEC_ERR_DEVICE, c.err);
  return CTCDEC_OK;
}
// ... and at the end of the host's work the call's own time; the result is the caller's from here on.
static void close_call(DecodeCall& c) {
  c.t_end = Clock::now();
  c.res->ms[2] = ms(c.t_begin, c.t_end);
  *c.out = c.res.release();
}

// 9a. One block of text per utterance, written by the kernels.
static int finish_device_texts(DecodeCall& c) {
  ctcdec_result* res = c.res.get();
  std::string& err = c.err;
  unsigned long long heads[2] = {c.heads_pinned[0], c.heads_pinned[1]};  // (read back with the counters)
  if (c.outgrown_redone && be::d2h(heads, c.dec->w_head.p, 16, &err)) return fail(CTCDEC_ERR_DEVICE, err);
  res->device_texts = true;
  res->dev_out.resize((size_t)c.n_utts);
  res->dev_texts.resize((size_t)heads[1]);
  if (be::d2h(res->dev_out.data(), c.dec->w_out.p, (size_t)c.n_utts * sizeof(OutBeam), &err) ||
      (heads[1] && be::d2h(&res->dev_texts[0], c.dec->w_tpool.p, (size_t)heads[1], &err)))
    return fail(CTCDEC_ERR_DEVICE, err);
  for (int32_t u = 0; u < c.n_utts; ++u) {
    const OutBeam& ob = res->dev_out[(size_t)u];
    if (c.n_out[u] != 1 || (unsigned long long)ob.tok_off + ob.tok_cnt > heads[1]) return fail(CTCDEC_ERR_INTERNAL, "text pool range");
  }
  if (int rc = kernel_stats(c)) return rc;
  close_call(c);
  if (c.host_timing) {
    const PruneStage& s = c.prune;
    fprintf(stderr, "[ctcdec host] texts from the device: %llu bytes, native call %.3f ms (kernels %.3f + %.3f): setup %.3f, launches %.3f, "
                    "wait for the kernels %.3f, counters back %.3f, records + texts back %.3f\n", heads[1], res->ms[2], res->ms[0], res->ms[1],
            ms(c.t_begin, s.t_setup), ms(s.t_setup, s.t_queued), ms(s.t_queued, s.t_flags), ms(s.t_flags, c.t_kernel), ms(c.t_kernel, Clock::now()));
  }
  return CTCDEC_OK;
}

// 9b. A resident stream between reads: nothing to bring back.
static int finish_stream_push(DecodeCall& c) {
  const ctcdec_result* res = c.res.get();
  if (int rc = kernel_stats(c)) return rc;
  close_call(c);
  if (c.host_timing)
    fprintf(stderr, "[ctcdec host] stream push: setup+prune+launch %.3f ms, wait beam kernel %.3f ms, total %.3f ms (prune kernel %.3f, beam kernel %.3f)\n",
            ms(c.t_begin, c.t_launch), ms(c.t_launch, c.t_kernel), ms(c.t_begin, Clock::now()), res->ms[0], res->ms[1]);
  return CTCDEC_OK;
}

// 10. Token confidences: the tokens replay() has just listed go to the device as runs of rows of the survivor arrays, which
// this call's prune stage left there (whatever max_surv the overflow redo ended with), one kernel folds each run and one
// float64 per token comes back -- in the order of ctcdec_result_token_frames. A label that is missing from a frame's
// survivors is a broken invariant ("Token confidences"): the call fails, there is no substitute value.
static int stream_token_confidences(DecodeCall& c);
static int token_confidences(DecodeCall& c) {
  if (c.rs) return stream_token_confidences(c);
  ctcdec_decoder* dec = c.dec;
  ctcdec_result* res = c.res.get();
  std::string& err = c.err;
  const int max_surv = c.prune.max_surv;
  double logp_ms[3] = {0, 0, 0};  // pack + upload, kernel, download
  auto t0 = Clock::now();
  if (c.R > (int64_t)UINT32_MAX) return fail(CTCDEC_ERR_LIMIT, "token confidences: more than 2^32 frames in one call");
  size_t nt = 0;
  for (const auto& beams : res->utts)
    for (const BeamResult& b : beams) nt += b.tok.size() / 3;
  // (packed in page-locked memory that the decoder keeps: a fresh 20 MB of pageable memory costs more than the kernel)
  if (dec->h_truns.ensure(std::max<size_t>(nt, 1) * sizeof(TokRun), &err)) return fail(CTCDEC_ERR_DEVICE, err);
  TokRun* runs = (TokRun*)dec->h_truns.p;
  size_t o = 0;
  for (int32_t u = 0; u < c.n_utts; ++u)
    for (const BeamResult& b : res->utts[(size_t)u]) {
      const int32_t* t = b.tok.data();
      for (size_t k = 0, n = b.tok.size() / 3; k < n; ++k, ++o, t += 3) {
        const int64_t s = (int64_t)t[1] - c.p->first_frame, e = (int64_t)t[2] - c.p->first_frame;
        if (t[0] < 0 || t[0] >= c.V || s < 0 || e <= s || e > c.utt_frames[u]) return fail(CTCDEC_ERR_INTERNAL, "token frames out of range");
        runs[o] = TokRun{(uint32_t)(c.row0[(size_t)u] + s), (uint32_t)(e - s), (uint32_t)t[0]};
      }
    }
  res->tk_logp.resize(nt);
  uint32_t missing = 0;
#ifdef CTC_SIM  // (the simulator's device memory is host memory: the kernel's body, token by token)
  for (size_t i = 0; i < nt; ++i) {
    const uint32_t* cnt = (const uint32_t*)dec->w_scnt.p;
    const uint16_t* sid = (const uint16_t*)dec->w_sid.p;
    const double* slp = (const double*)dec->w_slp.p;
    missing += c.fold == LOGP_MEAN  ? token_logp_of<LOGP_MEAN>(runs[i], cnt, sid, slp, (uint32_t)max_surv, &res->tk_logp[i])
               : c.fold == LOGP_MIN ? token_logp_of<LOGP_MIN>(runs[i], cnt, sid, slp, (uint32_t)max_surv, &res->tk_logp[i])
                                    : token_logp_of<LOGP_MAX>(runs[i], cnt, sid, slp, (uint32_t)max_surv, &res->tk_logp[i]);
  }
  (void)t0;
#else
  if (nt) {
    if (dec->w_truns.ensure(nt * sizeof(TokRun), &err) || be::h2d(dec->w_truns.p, runs, nt * sizeof(TokRun), &err) ||
        dec->w_tlogp.ensure(nt * 8, &err) || dec->w_tmiss.ensure(16, &err) || be::zero(dec->w_tmiss.p, 16, &err))
      return fail(CTCDEC_ERR_DEVICE, err);
    be::TokenLogpArgs ta;
    ta.runs = (const TokRun*)dec->w_truns.p;
    ta.n_tokens = (int64_t)nt;
    ta.fold = c.fold;
    ta.surv_cnt = (const uint32_t*)dec->w_scnt.p;
    ta.surv_id = (const uint16_t*)dec->w_sid.p;
    ta.surv_lp = (const double*)dec->w_slp.p;
    ta.max_surv = max_surv;
    ta.out = (double*)dec->w_tlogp.p;
    ta.missing = (uint32_t*)dec->w_tmiss.p;
    auto t1 = Clock::now();
    if (be::launch_token_logp(ta, &err)) return fail(CTCDEC_ERR_DEVICE, err);
    if (c.host_timing) logp_ms[1] = be::last_token_logp_ms();
    auto t2 = Clock::now();
    if (be::d2h(res->tk_logp.data(), dec->w_tlogp.p, nt * 8, &err) || be::d2h(&missing, dec->w_tmiss.p, 4, &err))
      return fail(CTCDEC_ERR_DEVICE, err);
    logp_ms[0] = ms(t0, t1);
    logp_ms[2] = ms(t2, Clock::now());
  }
#endif
  if (missing)
    return fail(CTCDEC_ERR_INTERNAL, "token confidences: " + std::to_string(missing) + " token frames whose label is not among the frame's survivors");
  res->has_logp = true;
  if (c.host_timing)
    fprintf(stderr, "[ctcdec host] token confidences: %zu tokens, pack + upload %.3f ms, kernel %.3f ms, download %.3f ms\n", nt,
            logp_ms[0], logp_ms[1], logp_ms[2]);
  return CTCDEC_OK;
}

// ... of a device-resident stream: a token's frames may lie in any chunk pushed so far, so its run is rows of the stream's
// survivor ledger (row = frame - the stream's first frame) and token_logp_ledger<fold> folds it; the rest is the same.
static int stream_token_confidences(DecodeCall& c) {
  ctcdec_decoder* dec = c.dec;
  ctcdec_stream* rs = c.rs;
  ctcdec_result* res = c.res.get();
  std::string& err = c.err;
  if (!c.led || c.led != c.fold || c.led_rows.size() != (size_t)c.n_utts) return fail(CTCDEC_ERR_INTERNAL, "token confidences: the stream keeps no ledger");
  auto t0 = Clock::now();
  size_t nt = 0;
  for (const auto& beams : res->utts)
    for (const BeamResult& b : beams) nt += b.tok.size() / 3;
  if (dec->h_truns.ensure(std::max<size_t>(nt, 1) * sizeof(LedgerRun), &err)) return fail(CTCDEC_ERR_DEVICE, err);
  LedgerRun* runs = (LedgerRun*)dec->h_truns.p;
  size_t o = 0;
  for (int32_t u = 0; u < c.n_utts; ++u)
    for (const BeamResult& b : res->utts[(size_t)u]) {
      const int32_t* t = b.tok.data();
      for (size_t k = 0, n = b.tok.size() / 3; k < n; ++k, ++o, t += 3) {
        const int64_t s = (int64_t)t[1] - rs->led_first[(size_t)u], e = (int64_t)t[2] - rs->led_first[(size_t)u];
        if (t[0] < 0 || t[0] >= c.V || s < 0 || e <= s || e > c.led_rows[(size_t)u]) return fail(CTCDEC_ERR_INTERNAL, "token frames out of range");
        runs[o] = LedgerRun{(uint32_t)u, (uint32_t)s, (uint32_t)(e - s), (uint32_t)t[0]};
      }
    }
  res->tk_logp.resize(nt);
  uint32_t missing = 0;
  double kernel_ms = 0;
#ifdef CTC_SIM  // (the simulator's device memory is host memory: the kernel's body, token by token)
  for (size_t i = 0; i < nt; ++i) {
    const size_t u = runs[i].stream;
    const uint64_t* ro = (const uint64_t*)rs->led_off.p + u * (rs->led_row_cap + 1);
    const uint16_t* id = (const uint16_t*)rs->led_id.p + u * rs->led_ent_cap;
    const double* lp = (const double*)rs->led_lp.p + u * rs->led_ent_cap;
    missing += c.fold == LOGP_MEAN  ? ledger_logp_of<LOGP_MEAN>(runs[i], ro, id, lp, &res->tk_logp[i])
               : c.fold == LOGP_MIN ? ledger_logp_of<LOGP_MIN>(runs[i], ro, id, lp, &res->tk_logp[i])
                                    : ledger_logp_of<LOGP_MAX>(runs[i], ro, id, lp, &res->tk_logp[i]);
  }
#else
  if (nt) {
    if (dec->w_truns.ensure(nt * sizeof(LedgerRun), &err) || be::h2d(dec->w_truns.p, runs, nt * sizeof(LedgerRun), &err) ||
        dec->w_tlogp.ensure(nt * 8, &err) || dec->w_tmiss.ensure(16, &err) || be::zero(dec->w_tmiss.p, 16, &err))
      return fail(CTCDEC_ERR_DEVICE, err);
    be::LedgerLogpArgs ta;
    ta.runs = (const LedgerRun*)dec->w_truns.p;
    ta.n_tokens = (int64_t)nt;
    ta.fold = c.fold;
    ta.row_off = (const uint64_t*)rs->led_off.p;
    ta.id = (const uint16_t*)rs->led_id.p;
    ta.lp = (const double*)rs->led_lp.p;
    ta.row_cap = rs->led_row_cap;
    ta.ent_cap = rs->led_ent_cap;
    ta.out = (double*)dec->w_tlogp.p;
    ta.missing = (uint32_t*)dec->w_tmiss.p;
    if (be::launch_ledger_logp(ta, &err)) return fail(CTCDEC_ERR_DEVICE, err);
    if (c.host_timing) kernel_ms = be::last_ledger_logp_ms();
    if (be::d2h(res->tk_logp.data(), dec->w_tlogp.p, nt * 8, &err) || be::d2h(&missing, dec->w_tmiss.p, 4, &err))
      return fail(CTCDEC_ERR_DEVICE, err);
  }
#endif
  if (missing)
    return fail(CTCDEC_ERR_INTERNAL, "token confidences: " + std::to_string(missing) + " token frames whose label is not in the frame's ledger row");
  res->has_logp = true;
  if (c.host_timing)
    fprintf(stderr, "[ctcdec host] stream token confidences: %zu tokens, token_logp_ledger kernel %.3f ms, all of it %.3f ms\n", nt, kernel_ms,
            ms(t0, Clock::now()));
  return CTCDEC_OK;
}

// 9c. The full result: output records, emission lists and the further models' states back, then the host replay.
static int finish_beams(DecodeCall& c) {
  ctcdec_decoder* dec = c.dec;
  ctcdec_result* res = c.res.get();
  std::string& err = c.err;
  const int32_t n_utts = c.n_utts;
  const int n_best = c.n_best, K = c.K;
  const unsigned long long head = c.head;
  const OutBeam* obs = (const OutBeam*)dec->h_out.p;
  if (be::d2h(dec->h_out.p, dec->w_out.p, (size_t)n_utts * n_best * sizeof(OutBeam), &err))
    return fail(CTCDEC_ERR_DEVICE, err);
  if (dec->h_tok.ensure((size_t)head * sizeof(EmitNode) + 16, &err)) return fail(CTCDEC_ERR_DEVICE, err);
  const EmitNode* toks = (const EmitNode*)dec->h_tok.p;
  if (head && be::d2h(dec->h_tok.p, dec->w_tok.p, (size_t)head * sizeof(EmitNode), &err))
    return fail(CTCDEC_ERR_DEVICE, err);
  const LmState* xst = nullptr;
  if (c.xstate_bytes) {
    if (dec->h_xstate.ensure(c.xstate_bytes, &err) || be::d2h(dec->h_xstate.p, dec->w_xstate.p, c.xstate_bytes, &err))
      return fail(CTCDEC_ERR_DEVICE, err);
    xst = (const LmState*)dec->h_xstate.p;
  }
  auto t_copy = Clock::now();
  if (int rc = kernel_stats(c)) return rc;
  for (int32_t u = 0; u < n_utts; ++u)
    for (uint32_t k = 0; k < c.n_out[u]; ++k) {
      const OutBeam& ob = obs[(size_t)u * n_best + k];
      if ((unsigned long long)ob.tok_off + ob.tok_cnt > head) return fail(CTCDEC_ERR_INTERNAL, "token pool range");
    }
  const bool want_tok = c.p->token_frames != 0;
  const StreamIn* stream = c.stream;
  res->has_tokens = want_tok;
  auto replay_range = [&](int32_t u0, int32_t u1) {
    for (int32_t u = u0; u < u1; ++u) {
      auto& beams = res->utts[(size_t)u];
      beams.resize(c.n_out[u]);
      for (uint32_t k = 0; k < c.n_out[u]; ++k) {
        const OutBeam& ob = obs[(size_t)u * n_best + k];
        BeamResult& r = beams[k];
        fill_result(ob, xst ? &xst[((size_t)u * n_best + k) * (size_t)(K - 1)] : nullptr, K, &r);
        replay(dec, toks + ob.tok_off, ob.tok_cnt, stream, stream ? stream->beam_off[u] : 0, &r, want_tok, (int32_t)ob.pad[0],
               (int32_t)ob.pad[1]);
      }
    }
  };
  // host replay is independent per utterance: a few threads once there is enough of it
  if (head > 50000 && n_utts >= 16) {
    if (!dec->replay_pool) {
      unsigned want = 31u;  // + the calling thread
      if (const char* env = getenv("CTCDEC_REPLAY_THREADS")) want = (unsigned)std::max(0, atoi(env) - 1);
      const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
      dec->replay_pool.reset(new ReplayPool((int)std::min(want, hw > 1 ? hw - 1 : 0u)));
    }
    const std::function<void(int32_t, int32_t)> job = replay_range;
    dec->replay_pool->run(n_utts, 4, job);
  } else {
    replay_range(0, n_utts);
  }
  if (c.fold)
    if (int rc = token_confidences(c)) return rc;
  close_call(c);
  if (c.host_timing)
    fprintf(stderr, "[ctcdec host] setup+launch %.3f ms, wait kernels %.3f ms, copy back %.3f ms (%llu tokens), replay %.3f ms\n",
            ms(c.t_begin, c.t_launch), ms(c.t_launch, c.t_kernel), ms(c.t_kernel, t_copy), head, ms(t_copy, c.t_end));
  return CTCDEC_OK;
}

static int decode_impl(ctcdec_decoder* dec, const void* const* utt_logits, const int32_t* utt_frames, int32_t n_utts,
                       int32_t dtype, int32_t is_device, const ctcdec_params* p, const ctcdec_lm_state* start_states,
                       const DecodeMode& mode, ctcdec_result** out) {
  DecodeCall c{mode, dec, p, utt_logits, utt_frames, start_states, out, n_utts, dtype, is_device};
  if (int rc = check_call(c)) return rc;
  if (n_utts == 0) {  // (nothing to decode: no device lock, no tables)
    *out = c.res.release();
    return CTCDEC_OK;
  }
  if (int rc = open_call(c)) return rc;
  if (int rc = stage_logits(c)) return rc;
  c.arenas_full = c.rs != nullptr || dec->arenas_worst_case || getenv("CTCDEC_WORST_CASE_ARENAS") != nullptr;
  size_arenas(c, c.arenas_full);
  if (int rc = c.rs ? stage_resident_input(c) : c.stream ? stage_imports(c) : CTCDEC_OK) return rc;
  if (int rc = reserve_beam_workspace(c)) return rc;
  if (int rc = stage_start_states(c)) return rc;
  if (int rc = fill_beam_args(c)) return rc;
  if (int rc = prune_and_launch(c)) return rc;
  if (c.after_launch && *c.after_launch && (*c.after_launch)(&c.err)) return fail(CTCDEC_ERR_DEVICE, c.err);
  if (int rc = collect_counters(c)) return rc;
  return c.device_texts ? finish_device_texts(c) : c.want_result ? finish_beams(c) : finish_stream_push(c);
}

// ---- device-resident streams ------------------------------------------------------------------------------------
int ctcdec_stream_open(ctcdec_decoder* dec, int32_t n_streams, const ctcdec_lm_state* start_states, ctcdec_stream** out) {
  if (!dec || !out || n_streams < 1) return fail(CTCDEC_ERR_ARG, "bad arguments");
  std::string err;
  std::lock_guard<std::mutex> device_lock(g_device_mu);
  if (be::bind_thread(&err)) return fail(CTCDEC_ERR_DEVICE, err);
  std::unique_ptr<ctcdec_stream> st(new ctcdec_stream());
  st->dec = dec;
  st->n = n_streams;
  st->K = dec->has_lm ? dec->n_lms() : 1;
  if (start_states && dec->has_lm) st->start_states.assign(start_states, start_states + (size_t)n_streams * st->K);
  st->mirror.assign((size_t)n_streams, StreamState{0u, 1u, 0u, 0u});
  st->frames.assign((size_t)n_streams, 0);
  st->imp_off.assign((size_t)n_streams + 1, 0);
  if (st->carry.ensure((size_t)n_streams * ctcdec_stream::CAP * sizeof(ImportBeam), &err) ||
      (st->K > 1 && st->carry_x.ensure((size_t)n_streams * ctcdec_stream::CAP * (size_t)(st->K - 1) * sizeof(LmState), &err)) ||
      // (behind the counters: room for a survivor ledger's entry counts and its overrun word, read back with them)
      st->sstate.ensure((size_t)n_streams * (sizeof(StreamState) + 8) + 8, &err) ||
      be::h2d(st->sstate.p, st->mirror.data(), (size_t)n_streams * sizeof(StreamState), &err))
    return fail(CTCDEC_ERR_DEVICE, err);
  *out = st.release();
  return CTCDEC_OK;
}

int ctcdec_stream_push(ctcdec_stream* st, const void* const* chunk_logits, const int32_t* chunk_frames, int32_t dtype,
                       int32_t is_device, const ctcdec_params* params, const int32_t* first_frame, int32_t force_next_word,
                       int32_t is_end, int32_t want_result, ctcdec_result** out) {
  if (!st || !params || !chunk_frames) return fail(CTCDEC_ERR_ARG, "bad arguments");
  if ((want_result || is_end) && !out) return fail(CTCDEC_ERR_ARG, "a result is wanted but there is nowhere to put it");
  std::vector<int32_t> ff((size_t)st->n);
  // (a stream with a survivor ledger numbers its frames from its first chunk's first_frame)
  const bool led = st->led_fold != 0 && st->pushes > 0;
  for (int32_t u = 0; u < st->n; ++u)
    ff[(size_t)u] = first_frame ? first_frame[u] : (int32_t)st->frames[(size_t)u] + (led ? st->led_first[(size_t)u] : 0);
  const StreamIn sin{ff.data(), st->has_import ? st->imp_beams.data() : nullptr, st->imp_off.data(), st->imp_blob.data(),
                     (force_next_word || is_end) ? 1 : 0, is_end ? 1 : 0};
  ctcdec_result* res = nullptr;
  HotCallScope hot_scope(st->dec);
  const int rc = decode_impl(st->dec, chunk_logits, chunk_frames, st->n, dtype, is_device, params,
                             st->start_states.empty() ? nullptr : st->start_states.data(),
                             DecodeMode{&sin, st, want_result != 0 || is_end != 0}, &res);
  if (rc != CTCDEC_OK) return rc;
  if (out) *out = res;
  else ctcdec_result_free(res);
  return CTCDEC_OK;
}

int ctcdec_stream_read(ctcdec_stream* st, const ctcdec_params* params, ctcdec_result** out) {
  if (!st || !params || !out) return fail(CTCDEC_ERR_ARG, "bad arguments");
  // a chunk of zero frames: the finalisation ranks the carried beams again (same beams, same order) and this time
  // writes output records and back-traces the emission chains
  std::vector<const void*> ptrs((size_t)st->n, nullptr);
  std::vector<int32_t> zero((size_t)st->n, 0);
  return ctcdec_stream_push(st, ptrs.data(), zero.data(), CTCDEC_F32, 0, params, nullptr, 0, 0, 1, out);
}

int ctcdec_stream_import(ctcdec_stream* st, const ctcdec_beam_in* beams, const int64_t* beam_off, const char* text_blob,
                         int64_t text_bytes) {
  if (!st || !beams || !beam_off || !text_blob || text_bytes < 0) return fail(CTCDEC_ERR_ARG, "bad arguments");
  ctcdec_decoder* dec = st->dec;
  HotCallScope hot_scope(dec);
  if (dec->hot_call.armed) {
    if ((int32_t)dec->hot_call.utt_set.size() != st->n) return fail(CTCDEC_ERR_ARG, "hot-word sets armed for another number of streams");
    build_hot_sets(dec->hot_call);
  }
  std::string err;
  std::lock_guard<std::mutex> device_lock(g_device_mu);
  if (be::bind_thread(&err)) return fail(CTCDEC_ERR_DEVICE, err);
  if (sync_tables(dec, &err)) return fail(CTCDEC_ERR_DEVICE, err);  // (the hot-word view of the partial words)
  const int K = st->K;
  const StreamIn sin{nullptr, beams, beam_off, text_blob, 0, 0};
  std::vector<ImportBeam> imps((size_t)st->n * ctcdec_stream::CAP);
  std::vector<LmState> imps_x(K > 1 ? imps.size() * (size_t)(K - 1) : 0);
  for (int32_t u = 0; u < st->n; ++u) {
    const int64_t cnt = beam_off[u + 1] - beam_off[u];
    if (cnt < 1 || cnt > ctcdec_stream::CAP) return fail(CTCDEC_ERR_ARG, "a stream must carry between 1 and 256 beams");
    for (int64_t k = 0; k < cnt; ++k) {
      const size_t slot = (size_t)u * ctcdec_stream::CAP + (size_t)k;
      std::string e = build_import(dec, sin, beam_off[u] + k, &imps[slot], K > 1 ? &imps_x[slot * (size_t)(K - 1)] : nullptr,
                                   import_hot(dec, u));
      if (!e.empty()) return fail(CTCDEC_ERR_ARG, e);
    }
  }
  // the new roots go behind what the arena already holds; the old chains are unreachable from now on
  for (int32_t u = 0; u < st->n; ++u) st->mirror[(size_t)u].n_carry = (uint32_t)(beam_off[u + 1] - beam_off[u]);
  if (be::h2d(st->carry.p, imps.data(), imps.size() * sizeof(ImportBeam), &err) ||
      (K > 1 && be::h2d(st->carry_x.p, imps_x.data(), imps_x.size() * sizeof(LmState), &err)) ||
      be::h2d(st->sstate.p, st->mirror.data(), (size_t)st->n * sizeof(StreamState), &err))
    return fail(CTCDEC_ERR_DEVICE, err);
  const int64_t nb = beam_off[st->n];
  st->imp_beams.assign(beams, beams + nb);
  for (auto& b : st->imp_beams) b.more_states = nullptr;  // (copied into the carry rows above)
  st->imp_off.assign(beam_off, beam_off + st->n + 1);
  st->imp_blob.assign(text_blob, (size_t)text_bytes);
  st->has_import = true;
  return CTCDEC_OK;
}

// ---- time-sliced ingest of host batches --------------------------------------------------------------------------------
// The reference is called with numpy matrices (decoder.py:730-775). Copying a large host batch takes longer than decoding it
// (2.1 GB: 37 ms over PCIe, 13 ms of kernels), and an utterance's beam search is ~11 us x T of latency whatever the batch size,
// so overlapping per-utterance chunks would still end with one full-length decode after the last copy. TIME slices do not:
// the batch goes through the device-resident stream machinery (ctcdec_stream_*: the beams stay on the device between
// slices), slice k + 1 is copied -- hipMemcpy2D of [utterances x slice bytes] with the batch's pitch, as fast from pageable
// memory as one big copy: tools/h2d_2d_probe.py -- while slice k's kernels run, and only the last slice's kernels are exposed.
// Chunked == unchunked for logits (what partial_decode_beams guarantees and the suites check); the one thing that is a property
// of the WHOLE utterance is the probability sniff (decoder.py:760): whenever any slice of any utterance is within reach of
// "mean row sum = 1", or an utterance has slices on both sides of 1, the batch is decoded again in one piece (return 1).
static int host_slices_wanted(const ctcdec_decoder* dec, const int32_t* utt_frames, int32_t n_utts, int32_t dtype) {
  const char* env = getenv("CTCDEC_HOST_SLICES");  // 0: never; n >= 2: always, in n slices (tests); unset: by size
  if (env && atoi(env) < 2) return 0;
  const size_t esz = dtype_size(dtype);
  int64_t rows = 0, tmax = 0;
  for (int32_t u = 0; u < n_utts; ++u) {
    if (utt_frames[u] < 0) return 0;
    rows += utt_frames[u];
    tmax = std::max<int64_t>(tmax, utt_frames[u]);
  }
  const double bytes = (double)rows * (double)dec->alpha.labels.size() * (double)esz;
  int n = env ? atoi(env) : (bytes >= 512e6 ? (int)std::min(16.0, std::max(4.0, bytes / 256e6)) : 0);
  if (n > tmax / 2) n = (int)(tmax / 2);
  return n >= 2 ? n : 0;
}

static int decode_host_sliced(ctcdec_decoder* dec, const void* const* utt_logits, const int32_t* utt_frames, int32_t n_utts,
                              int32_t dtype, const ctcdec_params* p, const ctcdec_lm_state* start_states, int n_slices,
                              ctcdec_result** out) {
  if (p->beam_width < 1 || p->beam_width > CTCDEC_MAX_BEAM_WIDTH) return 1;  // (the one-piece path words the refusal)
  const size_t V = dec->alpha.labels.size();
  const size_t esz = dtype_size(dtype);
  int64_t tmax = 0;
  for (int32_t u = 0; u < n_utts; ++u) tmax = std::max<int64_t>(tmax, utt_frames[u]);
  const int64_t C = (tmax + n_slices - 1) / n_slices;  // frames per slice
  const size_t row_bytes = V * esz, slot = (size_t)C * row_bytes;
  std::string err;
  ctcdec_stream* st = nullptr;
  int rc = ctcdec_stream_open(dec, n_utts, start_states, &st);
  if (rc != CTCDEC_OK) return rc;
  // per utterance: "a slice was read as probabilities" (u32), then the sum of all row sums seen so far (f64)
  const size_t side_off = ((size_t)n_utts * 4 + 15) & ~(size_t)15, side_bytes = side_off + (size_t)n_utts * 8;
  struct Closer {
    ctcdec_stream* s;
    ctcdec_decoder* d;
    ~Closer() {
      d->slicing = false;
      ctcdec_stream_close(s);
    }
  } closer{st, dec};
  {
    std::lock_guard<std::mutex> device_lock(g_device_mu);
    if (be::bind_thread(&err) || dec->w_logits.ensure(2 * (size_t)n_utts * slot, &err) || dec->w_side.ensure(side_bytes, &err) ||
        be::zero(dec->w_side.p, side_bytes, &err) || be::sync(&err))
      return fail(CTCDEC_ERR_DEVICE, err);
  }
  dec->slicing = true;
  std::vector<int32_t> frames((size_t)n_utts);
  std::vector<const void*> ptrs((size_t)n_utts);
  auto slice_frames = [&](int k, int32_t u) { return (int32_t)std::max<int64_t>(0, std::min<int64_t>(C, (int64_t)utt_frames[u] - (int64_t)k * C)); };
  // slice k of every utterance -> half (k & 1) of the staging buffer, utterance u at u * slot: runs of utterances that follow
  // each other in host memory with one length (a [B, T, V] array) go over in ONE two-dimensional copy
  auto copy_slice = [&](int k, std::string* e) -> int {
    char* half = (char*)dec->w_logits.p + (size_t)(k & 1) * (size_t)n_utts * slot;
    for (int32_t u = 0; u < n_utts;) {
      const int32_t f = slice_frames(k, u);
      int32_t v = u + 1;
      const size_t pitch = (size_t)utt_frames[u] * row_bytes;
      while (v < n_utts && utt_frames[v] == utt_frames[u] && (const char*)utt_logits[v] == (const char*)utt_logits[u] + (size_t)(v - u) * pitch) ++v;
      if (f > 0 && be::h2d_2d_overlapped(half + (size_t)u * slot, slot, (const char*)utt_logits[u] + (size_t)k * slot, pitch,
                                         (size_t)f * row_bytes, (size_t)(v - u), e))
        return -1;
      u = v;
    }
    return 0;
  };
  const bool trace = getenv("CTCDEC_SLICE_TRACE") != nullptr;
  if (trace) fprintf(stderr, "[ctcdec host] time-sliced ingest: %d utterances, %d slices of %lld frames\n", n_utts, n_slices, (long long)C);
  if (copy_slice(0, &err)) return fail(CTCDEC_ERR_DEVICE, err);
  ctcdec_result* res = nullptr;
  for (int k = 0; k < n_slices; ++k) {
    const bool last = k == n_slices - 1;
    char* half = (char*)dec->w_logits.p + (size_t)(k & 1) * (size_t)n_utts * slot;
    for (int32_t u = 0; u < n_utts; ++u) {
      frames[(size_t)u] = slice_frames(k, u);
      ptrs[(size_t)u] = half + (size_t)u * slot;
    }
    std::vector<int32_t> ff((size_t)n_utts);
    for (int32_t u = 0; u < n_utts; ++u) ff[(size_t)u] = (int32_t)st->frames[(size_t)u];
    const StreamIn sin{ff.data(), nullptr, st->imp_off.data(), st->imp_blob.data(), last ? 1 : 0, last ? 1 : 0};
    const AfterLaunch next = [&, k](std::string* e) -> int { return copy_slice(k + 1, e); };
    res = nullptr;
    rc = decode_impl(dec, ptrs.data(), frames.data(), n_utts, dtype, /*is_device=*/1, p,
                     st->start_states.empty() ? nullptr : st->start_states.data(),
                     DecodeMode{&sin, st, /*want_result=*/last, last ? nullptr : &next}, &res);
    if (rc != CTCDEC_OK) return rc;
    if (!last) ctcdec_result_free(res);
  }
  // The probability test (decoder.py:760) is about the whole utterance: the sliced decode stands when no slice was read as
  // probabilities AND the utterance's own mean row sum is safely not 1 (the slices' sums carry float32 noise of < 1e-2 per row:
  // 0.05 is far outside it and far inside what logits give) -- else the batch is decoded again in one piece.
  std::vector<unsigned char> side(side_bytes, 0);
  {
    std::lock_guard<std::mutex> device_lock(g_device_mu);
    if (be::bind_thread(&err) || be::d2h(side.data(), dec->w_side.p, side_bytes, &err)) {
      ctcdec_result_free(res);
      return fail(CTCDEC_ERR_DEVICE, err);
    }
  }
  const uint32_t* seen = (const uint32_t*)side.data();
  const double* sums = (const double*)(side.data() + side_off);
  for (int32_t u = 0; u < n_utts; ++u) {
    const double mean = utt_frames[u] > 0 ? sums[u] / (double)utt_frames[u] : NAN;
    if (seen[u] == 3u || (std::isfinite(mean) && fabs(mean - 1.0) <= 0.05)) {
      if (trace) fprintf(stderr, "[ctcdec host] time-sliced ingest: probability-like rows, decoding in one piece\n");
      ctcdec_result_free(res);
      return 1;
    }
  }
  *out = res;
  return CTCDEC_OK;
}

int ctcdec_stream_frames(const ctcdec_stream* st, int64_t* frames_out) {
  if (!st || !frames_out) return fail(CTCDEC_ERR_ARG, "bad arguments");
  for (int32_t u = 0; u < st->n; ++u) frames_out[u] = st->frames[(size_t)u];
  return CTCDEC_OK;
}

int ctcdec_stream_ledger_bytes(const ctcdec_stream* st, int64_t* bytes_out) {
  if (!st || !bytes_out) return fail(CTCDEC_ERR_ARG, "bad arguments");
  *bytes_out = (int64_t)st->led_bytes();
  return CTCDEC_OK;
}

void ctcdec_stream_close(ctcdec_stream* st) {
  if (!st) return;
  std::string err;
  std::lock_guard<std::mutex> device_lock(g_device_mu);
  be::bind_thread(&err);
  delete st;
}

// Diagnostics: run only the frame-prune stage on one utterance and hand back its survivor lists.
int ctcdec_frame_survivors(ctcdec_decoder* dec, const void* logits, int32_t n_frames, int32_t dtype, int32_t is_device,
                           double token_min_logp, int32_t stride, int32_t* counts, int32_t* ids, double* logps) {
  if (!dec || !counts || !ids || !logps || n_frames < 0 || stride < 1 || (n_frames > 0 && !logits))
    return fail(CTCDEC_ERR_ARG, "bad arguments");
  if (dtype < CTCDEC_F32 || dtype > CTCDEC_BF16) return fail(CTCDEC_ERR_ARG, "dtype must be f32, f64, f16 or bf16");
  if (n_frames == 0) return CTCDEC_OK;
  std::string err;
  std::lock_guard<std::mutex> device_lock(g_device_mu);
  if (be::bind_thread(&err)) return fail(CTCDEC_ERR_DEVICE, err);
  const int V = (int)dec->alpha.labels.size();
  const size_t esz = dtype_size(dtype);
  const size_t rows = (size_t)n_frames;
  std::vector<const void*> ptrs(1, logits);
  if (!is_device) {
    if (dec->w_logits.ensure(rows * V * esz, &err) || be::h2d(dec->w_logits.p, logits, rows * V * esz, &err))
      return fail(CTCDEC_ERR_DEVICE, err);
    ptrs[0] = dec->w_logits.p;
  }
  std::vector<int64_t> row0 = {0, (int64_t)n_frames};
  if (upload(dec->w_ptrs, ptrs, &err) || upload(dec->w_row0, row0, &err)) return fail(CTCDEC_ERR_DEVICE, err);
  PruneStage s{dec, &ptrs, 1, dtype, n_frames, V, token_min_logp};  // the decode's own prune stage, no beam stage behind it
  if (int rc = prune_stage(s, nullptr)) return rc;
  const size_t max_surv = (size_t)s.max_surv;
  std::vector<uint32_t> cnt(rows);
  std::vector<uint16_t> sid(rows * max_surv);
  std::vector<double> slp(rows * max_surv);
  if (be::d2h(cnt.data(), dec->w_scnt.p, rows * 4, &err) || be::d2h(sid.data(), dec->w_sid.p, sid.size() * 2, &err) ||
      be::d2h(slp.data(), dec->w_slp.p, slp.size() * 8, &err))
    return fail(CTCDEC_ERR_DEVICE, err);
  for (size_t t = 0; t < rows; ++t) {
    counts[t] = (int32_t)cnt[t];
    for (uint32_t k = 0; k < cnt[t] && k < (uint32_t)stride; ++k) {
      ids[t * (size_t)stride + k] = sid[t * max_surv + k];
      logps[t * (size_t)stride + k] = slp[t * max_surv + k];
    }
  }
  return CTCDEC_OK;
}

// a texts-only result (params.texts_only) as ordinary beams, for the accessors that want them
static void materialise(const ctcdec_result* cr) {
  ctcdec_result* r = const_cast<ctcdec_result*>(cr);
  if (!r || !r->device_texts || r->dev_out.empty()) return;
  for (size_t u = 0; u < r->dev_out.size(); ++u) {
    const OutBeam& ob = r->dev_out[u];
    r->utts[u].resize(1);
    BeamResult& b = r->utts[u][0];
    b.text.assign(r->dev_texts, ob.tok_off, ob.tok_cnt);
    b.logit = ob.logit_score;
    b.lm = ob.lm_score;
    b.state.length = -1;
    for (int j = 0; j < MAX_CTX; ++j) {
      b.state.words[j] = 0;
      b.state.backoff[j] = 0.f;
    }
    b.word_off.assign(1, (int32_t)b.text.size());
  }
  r->dev_out.clear();
}
int32_t ctcdec_result_num_utts(const ctcdec_result* r) { return r ? (int32_t)r->utts.size() : 0; }
int32_t ctcdec_result_num_beams(const ctcdec_result* r, int32_t utt) {
  materialise(r);
  if (!r || utt < 0 || (size_t)utt >= r->utts.size()) return 0;
  return (int32_t)r->utts[(size_t)utt].size();
}
static const BeamResult* get_beam(const ctcdec_result* r, int32_t utt, int32_t beam) {
  materialise(r);
  if (!r || utt < 0 || (size_t)utt >= r->utts.size()) return nullptr;
  const auto& b = r->utts[(size_t)utt];
  if (beam < 0 || (size_t)beam >= b.size()) return nullptr;
  return &b[(size_t)beam];
}
int ctcdec_result_text(const ctcdec_result* r, int32_t utt, int32_t beam, const char** s, int64_t* len) {
  const BeamResult* b = get_beam(r, utt, beam);
  if (!b) return fail(CTCDEC_ERR_ARG, "no such beam");
  *s = b->text.data();
  *len = (int64_t)b->text.size();
  return CTCDEC_OK;
}
int ctcdec_result_scores(const ctcdec_result* r, int32_t utt, int32_t beam, double* logit, double* lm) {
  const BeamResult* b = get_beam(r, utt, beam);
  if (!b) return fail(CTCDEC_ERR_ARG, "no such beam");
  *logit = b->logit;
  *lm = b->lm;
  return CTCDEC_OK;
}
int ctcdec_result_frames(const ctcdec_result* r, int32_t utt, int32_t beam, int32_t* n_words,
                         const int32_t** word_off, const int32_t** start, const int32_t** end) {
  const BeamResult* b = get_beam(r, utt, beam);
  if (!b) return fail(CTCDEC_ERR_ARG, "no such beam");
  *n_words = (int32_t)b->start.size();
  *word_off = b->word_off.data();
  *start = b->start.data();
  *end = b->end.data();
  return CTCDEC_OK;
}
int ctcdec_result_lm_state(const ctcdec_result* r, int32_t utt, int32_t beam, ctcdec_lm_state* out) {
  const BeamResult* b = get_beam(r, utt, beam);
  if (!b) return fail(CTCDEC_ERR_ARG, "no such beam");
  *out = b->state;
  return CTCDEC_OK;
}
int ctcdec_result_lm_state_of(const ctcdec_result* r, int32_t utt, int32_t beam, int32_t k, ctcdec_lm_state* out) {
  const BeamResult* b = get_beam(r, utt, beam);
  if (!b || !out) return fail(CTCDEC_ERR_ARG, "no such beam");
  if (k == 0) {
    *out = b->state;
    return CTCDEC_OK;
  }
  if (k < 0 || (size_t)k > b->xstates.size()) return fail(CTCDEC_ERR_ARG, "no such language model");
  *out = b->xstates[(size_t)k - 1];
  return CTCDEC_OK;
}
// decode_batch only wants the texts: one blob + offsets, nothing else is touched (packing the word frames of a
// 4096-utterance batch costs more than copying its results back from the device)
int ctcdec_result_texts(ctcdec_result* r, const char** blob_out, const int64_t** off_out, int64_t* n_out) {
  if (!r || !blob_out || !off_out || !n_out) return fail(CTCDEC_ERR_ARG, "no result");
  materialise(r);
  if (!r->texts_packed) {
    size_t nb = 0, bytes = 0;
    for (const auto& beams : r->utts)
      for (const BeamResult& b : beams) {
        ++nb;
        bytes += b.text.size();
      }
    r->t_blob.clear();
    r->t_blob.reserve(bytes);
    r->t_off.clear();
    r->t_off.reserve(nb + 1);
    r->t_off.push_back(0);
    for (const auto& beams : r->utts)
      for (const BeamResult& b : beams) {
        r->t_blob += b.text;
        r->t_off.push_back((int64_t)r->t_blob.size());
      }
    r->texts_packed = true;
  }
  *blob_out = r->t_blob.data();
  *off_out = r->t_off.data();
  *n_out = (int64_t)r->t_off.size() - 1;
  return CTCDEC_OK;
}

int ctcdec_result_texts_joined(ctcdec_result* r, char sep, const char** blob_out, int64_t* bytes_out, int64_t* n_out) {
  if (!r || !blob_out || !bytes_out || !n_out) return fail(CTCDEC_ERR_ARG, "no result");
  if (r->device_texts && !r->dev_out.empty()) {  // straight from the blocks the device wrote
    r->j_blob.clear();
    r->j_blob.reserve(r->dev_texts.size() + r->dev_out.size());
    for (size_t u = 0; u < r->dev_out.size(); ++u) {
      if (u) r->j_blob += sep;
      r->j_blob.append(r->dev_texts, r->dev_out[u].tok_off, r->dev_out[u].tok_cnt);
    }
    *blob_out = r->j_blob.data();
    *bytes_out = (int64_t)r->j_blob.size();
    *n_out = (int64_t)r->dev_out.size();
    return CTCDEC_OK;
  }
  size_t nb = 0, bytes = 0;
  for (const auto& beams : r->utts)
    for (const BeamResult& b : beams) {
      ++nb;
      bytes += b.text.size() + 1;
    }
  r->j_blob.clear();
  r->j_blob.reserve(bytes);
  size_t k = 0;
  for (const auto& beams : r->utts)
    for (const BeamResult& b : beams) {
      if (k++) r->j_blob += sep;
      r->j_blob += b.text;
    }
  *blob_out = r->j_blob.data();
  *bytes_out = (int64_t)r->j_blob.size();
  *n_out = (int64_t)nb;
  return CTCDEC_OK;
}

int ctcdec_result_text_blocks(ctcdec_result* r, const char** pool_out, const int64_t** off_out, const int64_t** len_out,
                              int64_t* n_out) {
  if (!r || !pool_out || !off_out || !len_out || !n_out) return fail(CTCDEC_ERR_ARG, "no result");
  if (r->device_texts && !r->dev_out.empty()) {  // the blocks the device wrote, as they are
    if (r->blk_off.empty()) {
      r->blk_off.reserve(r->dev_out.size());
      r->blk_len.reserve(r->dev_out.size());
      for (const OutBeam& ob : r->dev_out) {
        r->blk_off.push_back((int64_t)ob.tok_off);
        r->blk_len.push_back((int64_t)ob.tok_cnt);
      }
    }
    *pool_out = r->dev_texts.data();
  } else {  // any other result: the packed texts
    const char* blob = nullptr;
    const int64_t* off = nullptr;
    int64_t n = 0;
    int rc = ctcdec_result_texts(r, &blob, &off, &n);
    if (rc != CTCDEC_OK) return rc;
    if (r->blk_off.empty() && n > 0) {
      r->blk_off.assign(off, off + n);
      for (int64_t i = 0; i < n; ++i) r->blk_len.push_back(off[i + 1] - off[i]);
    }
    *pool_out = blob;
  }
  *off_out = r->blk_off.data();
  *len_out = r->blk_len.data();
  *n_out = (int64_t)r->blk_off.size();
  return CTCDEC_OK;
}

int ctcdec_result_pack(ctcdec_result* r, ctcdec_packed* out) {
  if (!r || !out) return fail(CTCDEC_ERR_ARG, "no result");
  materialise(r);
  if (!r->packed) {
    size_t nb = 0, nw = 0, tb = 0;
    for (const auto& beams : r->utts)
      for (const BeamResult& b : beams) {
        ++nb;
        nw += b.start.size();
        tb += b.text.size();
      }
    r->text_blob.reserve(tb);
    r->text_off.reserve(nb + 1);
    r->word_cnt_off.reserve(nb + 1);
    r->partial_off.reserve(nb + 1);
    r->logit.reserve(nb);
    r->lm.reserve(nb);
    r->states.reserve(nb);
    r->src_beam.reserve(nb);
    r->last_char.reserve(nb);
    r->pstart.reserve(nb);
    r->pend.reserve(nb);
    r->raw_lm.reserve(nb);
    r->word_byte_off.reserve(nw);
    r->word_start.reserve(nw);
    r->word_end.reserve(nw);
    r->beam_off.assign(1, 0);
    r->text_off.assign(1, 0);
    r->word_cnt_off.assign(1, 0);
    r->partial_off.assign(1, 0);
    for (const auto& beams : r->utts) {
      for (const BeamResult& b : beams) {
        r->text_blob += b.text;
        r->text_off.push_back((int64_t)r->text_blob.size());
        r->logit.push_back(b.logit);
        r->lm.push_back(b.lm);
        r->states.push_back(b.state);
        r->partial_blob += b.partial;
        r->partial_off.push_back((int64_t)r->partial_blob.size());
        r->src_beam.push_back(b.src);
        r->last_char.push_back(b.last_char);
        r->pstart.push_back(b.pstart);
        r->pend.push_back(b.pend);
        r->raw_lm.push_back(b.raw_lm);
        for (size_t k = 0; k < b.start.size(); ++k) {
          r->word_byte_off.push_back(b.word_off[k]);
          r->word_start.push_back(b.start[k]);
          r->word_end.push_back(b.end[k]);
        }
        r->word_cnt_off.push_back((int64_t)r->word_start.size());
      }
      r->beam_off.push_back((int64_t)r->logit.size());
    }
    r->packed = true;
  }
  out->n_utts = (int64_t)r->utts.size();
  out->n_beams = (int64_t)r->logit.size();
  out->n_words = (int64_t)r->word_start.size();
  out->beam_off = r->beam_off.data();
  out->text_blob = r->text_blob.data();
  out->text_off = r->text_off.data();
  out->logit_score = r->logit.data();
  out->lm_score = r->lm.data();
  out->word_cnt_off = r->word_cnt_off.data();
  out->word_byte_off = r->word_byte_off.data();
  out->word_start = r->word_start.data();
  out->word_end = r->word_end.data();
  out->lm_state = r->states.data();
  out->partial_blob = r->partial_blob.data();
  out->partial_off = r->partial_off.data();
  out->src_beam = r->src_beam.data();
  out->last_char = r->last_char.data();
  out->partial_start = r->pstart.data();
  out->partial_end = r->pend.data();
  out->raw_lm_score = r->raw_lm.data();
  return CTCDEC_OK;
}

int ctcdec_result_token_frames(ctcdec_result* r, const int64_t** tok_off_out, const int32_t** label_out, const int32_t** start_out,
                               const int32_t** end_out, int64_t* n_tokens_out) {
  if (!r || !tok_off_out || !label_out || !start_out || !end_out || !n_tokens_out) return fail(CTCDEC_ERR_ARG, "no result");
  if (!r->has_tokens) return fail(CTCDEC_ERR_ARG, "the result was decoded without params.token_frames");
  if (!r->tok_packed) {
    size_t nb = 0, nt = 0;
    for (const auto& beams : r->utts)
      for (const BeamResult& b : beams) {
        ++nb;
        nt += b.tok.size() / 3;
      }
    r->tk_off.resize(nb + 1);
    r->tk_label.resize(nt);
    r->tk_start.resize(nt);
    r->tk_end.resize(nt);
    size_t j = 0, o = 0;
    r->tk_off[0] = 0;
    for (const auto& beams : r->utts)
      for (const BeamResult& b : beams) {
        const int32_t* t = b.tok.data();
        for (size_t k = 0, n = b.tok.size() / 3; k < n; ++k, ++o, t += 3) {
          r->tk_label[o] = t[0];
          r->tk_start[o] = t[1];
          r->tk_end[o] = t[2];
        }
        r->tk_off[++j] = (int64_t)o;
      }
    r->tok_packed = true;
  }
  *tok_off_out = r->tk_off.data();
  *label_out = r->tk_label.data();
  *start_out = r->tk_start.data();
  *end_out = r->tk_end.data();
  *n_tokens_out = (int64_t)r->tk_label.size();
  return CTCDEC_OK;
}

int ctcdec_result_token_logp(ctcdec_result* r, const double** logp_out, int64_t* n_tokens_out) {
  if (!r || !logp_out || !n_tokens_out) return fail(CTCDEC_ERR_ARG, "no result");
  if (!r->has_logp) return fail(CTCDEC_ERR_ARG, "the result was decoded without a token confidence fold (params.token_frames = CTCDEC_TOKEN_LOGP_*)");
  *logp_out = r->tk_logp.data();
  *n_tokens_out = (int64_t)r->tk_logp.size();
  return CTCDEC_OK;
}

int ctcdec_profile_phases(ctcdec_decoder* dec, int32_t enable, uint64_t* ticks_out, int32_t n) {
  if (!dec) return fail(CTCDEC_ERR_ARG, "bad arguments");
  dec->profile = enable != 0;
  if (ticks_out)
    for (int k = 0; k < n && k < N_PROF; ++k) ticks_out[k] = dec->prof[k];
  return CTCDEC_OK;
}

int ctcdec_result_timing(const ctcdec_result* r, double* ms3) {
  if (!r) return fail(CTCDEC_ERR_ARG, "no result");
  ms3[0] = r->ms[0];
  ms3[1] = r->ms[1];
  ms3[2] = r->ms[2];
  return CTCDEC_OK;
}
int ctcdec_result_beam_kernel(const ctcdec_result* r) { return r ? r->beam_kernel : 0; }
int ctcdec_device(void) { return be::current_device(); }
// Tearing down the per-beam strings and vectors of a large batch takes about as long as copying the results back from
// the device did: large results are handed to ONE reclaimer thread (started on first use, joined when the library is
// unloaded or the process exits, so that no free can race static destruction).
namespace {
class Reclaimer {
 public:
  ~Reclaimer() {
    {
      std::lock_guard<std::mutex> g(m_);
      stop_ = true;
    }
    cv_.notify_all();
    if (worker_.joinable()) worker_.join();
    for (ctcdec_result* r : queue_) delete r;
  }
  bool hand_over(ctcdec_result* r) {
    try {
      std::lock_guard<std::mutex> g(m_);
      if (stop_ || queue_.size() >= 64) return false;  // (a caller that frees faster than we reclaim: do it inline)
      if (!worker_.joinable()) worker_ = std::thread([this] { loop(); });
      queue_.push_back(r);
    } catch (...) {  // no thread / no memory: the caller frees inline (nothing may escape an extern "C" function)
      return false;
    }
    cv_.notify_one();
    return true;
  }

 private:
  void loop() {
    for (;;) {
      ctcdec_result* r = nullptr;
      {
        std::unique_lock<std::mutex> g(m_);
        cv_.wait(g, [this] { return stop_ || !queue_.empty(); });
        if (queue_.empty()) return;  // (stop requested and nothing left)
        r = queue_.back();
        queue_.pop_back();
      }
      delete r;
    }
  }
  std::mutex m_;
  std::condition_variable cv_;
  std::vector<ctcdec_result*> queue_;
  std::thread worker_;
  bool stop_ = false;
};
Reclaimer g_reclaimer;
}  // namespace

void ctcdec_result_free(ctcdec_result* r) {
  if (!r) return;
  if (r->utts.size() >= 256 && g_reclaimer.hand_over(r)) return;
  delete r;
}

}  // extern "C"

// The simulator is built from api.cpp alone (tests/sim/build_sim.py, tools/sim_sanitized.sh name it and not its neighbour):
// there the transcript calls come in with it. The library compiles api_transcript.cpp as a translation unit of its own.
#ifdef CTC_SIM
#include "api_transcript.cpp"
#endif
