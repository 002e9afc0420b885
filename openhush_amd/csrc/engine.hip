// engine.hip — ohw_state: activation buffers, KV caches and the stage drivers behind the C ABI
// (mel -> encoder -> cross K/V -> decoder steps -> device-side greedy loop).
//
// Replaces ctx.create_state() and the arithmetic inside state.full()
// (reference src/engine/whisper.rs:167-169, 266-268).
#include <execinfo.h>
#include <signal.h>
#include <unistd.h>

#include <cstring>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <type_traits>
#include <vector>
#include <algorithm>

#include "attention.hpp"
#include "dequant.hpp"
#include "gemm.hpp"
#include "kernels.hpp"
#include "logit_rules.hpp"
#include "model.hpp"

namespace ohw {
ohw_ctx* ctx_from_file(const char* path, int device, int dtype);
ohw_ctx* ctx_synthetic(const ohw_hparams* hp, uint32_t seed, int device, int dtype);
ohw_ctx* ctx_shell(const ohw_hparams* hp, int device, int dtype);
void select_device(int device);

thread_local std::string g_last_error;

// OHW_SEGV_TRACE=1 (diagnostics): print the native frames of a SIGSEGV before the default action takes the process down -
// the GPU debugger is not available on the pool, and a fault under a profiler or inside the runtime otherwise leaves nothing
namespace {
void segv_trace(int sig) {
  void* frames[64];
  const int n = backtrace(frames, 64);
  static const char msg[] = "\n[libohw] SIGSEGV, native frames:\n";
  (void)!write(2, msg, sizeof msg - 1);
  backtrace_symbols_fd(frames, n, 2);
  signal(sig, SIG_DFL);
  raise(sig);
}
struct SegvTraceInit {
  SegvTraceInit() {
    const char* e = getenv("OHW_SEGV_TRACE");
    if (e && *e == '1') signal(SIGSEGV, segv_trace);
  }
} g_segv_trace_init;
}  // namespace

static std::shared_mutex g_api_mu;
static thread_local int g_api_depth = 0;
ApiScope::ApiScope() { if (g_api_depth++ == 0) g_api_mu.lock_shared(); }
ApiScope::~ApiScope() { if (--g_api_depth == 0) g_api_mu.unlock_shared(); }
ApiRelease::ApiRelease() { if (g_api_depth > 0) g_api_mu.unlock_shared(); }
ApiRelease::~ApiRelease() { if (g_api_depth > 0) g_api_mu.lock_shared(); }
CaptureGate::CaptureGate() { g_api_mu.unlock_shared(); g_api_mu.lock(); }
CaptureGate::~CaptureGate() { g_api_mu.unlock(); g_api_mu.lock_shared(); }

template <typename F>
static int guard(F&& f) {
  ApiScope api;
  try {
    f();
    return OHW_OK;
  } catch (const Error& e) {
    g_last_error = e.what();
    return e.code;
  } catch (const std::bad_alloc&) {
    g_last_error = "host allocation failed";
    return OHW_E_OOM;
  } catch (const std::exception& e) {
    g_last_error = e.what();
    return OHW_E_TRANSCRIBE;
  } catch (...) {
    g_last_error = "unknown error";
    return OHW_E_TRANSCRIBE;
  }
}
}  // namespace ohw

using namespace ohw;

constexpr int DEC_KSPLIT_MAX = 8;   // most K-slices per output tile of a decoder RESID GEMM
static int env_int(const char* name, int dflt, int lo, int hi) {
  const char* e = getenv(name);
  if (!e || !*e) return dflt;
  const int v = atoi(e);
  return v < lo ? lo : v > hi ? hi : v;
}
// K-slices per output tile of the decoder's RESID GEMMs, read when a state is created (1 = no split, the default:
// with activation tiles mlp.2 takes 7.8 us unsplit, 7.6 us over 2 slices and 9.4 us over 4 - the hand-off costs
// about 3.5 us - so the split path is kept as a tuning knob for other shapes, exercised by the GPU tests)
static int dec_ksplit_long() { return env_int("OHW_DEC_KSPLIT_LONG", 1, 1, DEC_KSPLIT_MAX); }
static int dec_ksplit_short() { return env_int("OHW_DEC_KSPLIT_SHORT", 1, 1, DEC_KSPLIT_MAX); }


// the decoder GEMMs and the forms of their input, as ohw_dbg_counter names them ("dec_gemm.<gemm>[.<form>].<NT>x<MT>")
enum DecTallyGemm { DT_QKV, DT_O, DT_XQ, DT_XO, DT_FC1, DT_FC2, DT_LOGITS, DT_GEMMS };
enum DecTallyForm { DT_PLAIN, DT_LN, DT_PN, DT_KSPLIT, DT_FORMS };
static const char* const kDecTallyGemm[DT_GEMMS] = {"qkv", "o", "xq", "xo", "fc1", "fc2", "logits"};
static const char* const kDecTallyForm[DT_FORMS] = {"", ".ln", ".pn", ".ks"};
static const char* const kDecTallyShape[DG_N_SHAPES] = {"1x1", "2x1", "1x2", "2x2", "4x2", "1x6", "4x6", "5x6"};
static const char* const kXattnTally[XA_N_VARIANTS] = {"plain", "split", "rows2", "rows3", "rows4", "group2", "group3", "group4", "group5", "group_split"};
static const char* const kSelfAttnTally[4] = {"plain", "slots", "fused", "fused_slots"};

// OHW_DEBUG_MARKS=1: progress lines on stderr (which HIP call a tool died under)
#define BMARK(what, i) do { static const bool on_ = env_int("OHW_DEBUG_MARKS", 0, 0, 1) != 0; if (on_) { std::fprintf(stderr, "[ohw beam] %s %d\n", what, (int)(i)); std::fflush(stderr); } } while (0)

// The replayed iterations of the device decode loops, captured as hipGraphs.  Positions, tokens and the done flags live in
// device memory, so one capture serves every iteration of every call that agrees with it in GraphKey: what is baked into the
// captured launches.  A state keeps three caches (ohw_state: step_graphs, group_graphs, beam_graphs).
struct GraphKey {
  int rows = 0;        // decoder rows (step cache) or windows (group and beam caches)
  int group = 0;       // candidates (group cache) or beams (beam cache) per window; 0 in the step cache
  int cus = 0;         // CU budget of the stream
  int t_len = 0;       // audio context: a captured kernel argument
  bool var = false, invariant = false, persist = false;     // per-window contexts, the cross-attention variant rule, the persistent step
  bool flag = false;   // step cache: a temperature pass; beam cache: log-probability history on (other pointers baked in)
  bool phrases = false;   // a hot-phrase table is set: the iteration holds the boost kernel (which table is device data)
  bool repeat = false;    // the repetition rule is on: the iteration holds its kernel (the values are device data)
  bool commands = false;  // a command list is set: the iteration holds its kernel (list and penalty are device data)
  SamplerParams spar;  // compared byte by byte: fill_sampler zeroes the struct, padding included, before it fills it
  bool operator==(const GraphKey& o) const {
    return rows == o.rows && group == o.group && cus == o.cus && t_len == o.t_len && var == o.var && invariant == o.invariant &&
           persist == o.persist && flag == o.flag && phrases == o.phrases && repeat == o.repeat && commands == o.commands && std::memcmp(&spar, &o.spar, sizeof spar) == 0;
  }
};
// one entry = the graph of a key's iteration, or the PAIR of a key whose iterations alternate between two forms (beam search:
// the token-history and kv_slot double buffers); a pair is made, looked up and evicted together
struct GraphEntry {
  GraphKey key;
  hipGraph_t graph[2] = {nullptr, nullptr};
  hipGraphExec_t exec[2] = {nullptr, nullptr};
  void destroy() {
    for (int q = 0; q < 2; ++q) {
      if (exec[q]) (void)hipGraphExecDestroy(exec[q]);
      if (graph[q]) (void)hipGraphDestroy(graph[q]);
    }
  }
};
struct GraphCache {
  size_t capacity;
  bool marks = false;             // OHW_DEBUG_MARKS lines around the capture calls (the beam cache)
  int captures = 0;               // entries captured so far (ohw_dbg_counter: a second call with the same key adds none)
  std::vector<GraphEntry> entries;     // oldest first
  const GraphEntry* find(const GraphKey& key) const {
    for (const auto& e : entries)
      if (e.key == key) return &e;
    return nullptr;
  }
  // the entry of `key`, captured now if the cache does not hold it: body(q, capture_stream) enqueues iteration form q
  template <typename F> const GraphEntry& get_or_capture(ohw_state* st, const GraphKey& key, int n_graphs, F&& body);
  void clear() {
    for (auto& e : entries) e.destroy();
    entries.clear();
  }
};

struct ohw_state {
  ohw_ctx* ctx = nullptr;
  int max_batch = 0;
  int enc_batch = 0;  // windows of the decode batch the cross K/V holds (the last ohw_encode, or the total of its slices)
  int mel_batch = 0;  // windows of the last ohw_mel
  // reduced audio context (ohw_state_set_audio_ctx): encoder positions per window; 0 = the model's n_audio_ctx.  mel_ctx /
  // enc_ctx: the context the mel image / the cross K/V were made under - an encode or a decode under another one is refused
  int audio_ctx = 0, mel_ctx = 0, enc_ctx = 0;
  // per-window contexts inside that envelope (ohw_state_set_window_ctx).  win_ctx: the setting, one length per window of the next
  // mel / encode (empty: none); mel_win / enc_set: the setting the last mel / the last encode ran under; enc_win: the length of
  // every decode-batch slot the encodes recorded (valid while enc_var).  wc_enc mirrors win_ctx on the device (the mel and the
  // encoder's attention read it), wc_dec holds enc_win (every cross-attention reads it): the lengths are never launch arguments,
  // so a captured step serves every mix of one envelope
  std::vector<int32_t> win_ctx, mel_win, enc_set, enc_win;
  bool enc_var = false;
  DevBuf wc_enc, wc_dec;    // i32 [max_batch]
  // packed-row encoder (ohw_state_set_packed_encoder / OHW_ENC_PACKED=1; read at encode time, no effect without lengths): the
  // encoder runs on the sum of the lengths, the windows laid end to end.  pk_off: the windows' first packed rows (exclusive prefix
  // sum of wc_enc, then the row count); pk_map: packed row -> row b * envelope + t of the unpacked layout; both are filled on the
  // stream by every packed encode.  enc_pk: the host's copy of the last encode's offsets (empty: it ran unpacked) - ohw_state_fetch
  // unpacks the encoder taps with it.  enc_rows: rows of the last encode's dense GEMMs (ohw_dbg_counter "enc_rows")
  bool packed = false;
  DevBuf pk_off, pk_map;    // i32 [max_batch + 1], i32 [max_batch * n_audio_ctx]
  std::vector<int64_t> enc_pk;
  int64_t enc_rows = 0;
  // per-window language (ohw_state_set_window_lang).  lang_tab: one id per decode-batch slot, LANG_PENDING while it waits for a
  // detection; lang_prob: the soft-max rows the detection wrote.  The decodes build their prompt rows from lang_tab on the
  // device.  lang_kind is the host's whole knowledge of the table (empty: none set); lang_ids holds the explicit ids only
  enum LangKind : int8_t { LANG_EXPLICIT, LANG_WAITING, LANG_RESOLVED };
  std::vector<int8_t> lang_kind;
  std::vector<int32_t> lang_ids;      // explicit id, else LANG_PENDING: what an encode uploads again
  DevBuf lang_tab, lang_prob;         // i32 [max_batch], f32 [max_batch][n_langs]
  // per-window text context (ohw_state_set_window_prompt).  wp_len: the positions the context of every decode-batch slot occupies
  // (0, or its tokens + 1 for [prev]); empty: no table.  The table lives on the device, laid out as the prefill feeds it in chunks
  // of Q = wp_chunk positions (ohw_state_set_prefill_chunk: 8 or 16): wp_feed [chunk][table batch][Q] tokens ([eot] in the surplus
  // rows), wp_pos [chunk][max_batch] = Q * chunk, wp_lens [max_batch]; wp_done [chunk][max_batch] is the done mask of the prefill
  // under way (it depends on the call's active windows).  A 16-position chunk is not two adjacent 8-position chunks, so the host
  // keeps the contexts (wp_host: [prev] + tokens per slot) and lays the table out again when the chunk size changes
  std::vector<int32_t> wp_len;
  std::vector<std::vector<int32_t>> wp_host;
  DevBuf wp_feed, wp_pos, wp_done, wp_lens;
  int wp_chunks = 0;                 // chunks the buffers hold: ceil(n_text_ctx / 2 / 8)
  int wp_chunk = 8;                  // positions per prefill chunk
  bool prefill_xa = true;            // OHW_PREFILL_XA=0: the prefill's cross-attention through launch_cross_attn's kernels (A/B knob)
  int64_t tally_xchunk = 0;          // cross_attn_chunk_kernel launches (ohw_dbg_counter "xattn.chunk")
  bool gemm_small = false;  // OHW_GEMM_SMALL=1: short windows take the 64x64-tile encoder GEMM (gemm_small.hip; off until measured)
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  // front end
  DevBuf pcm, n_samples, logmel, max_bits, mel_t;
  DevBuf rec_pcm, rec_max, rec_off;   // a whole recording, the maximum of its log-mel spectrogram, window offsets (ohw_recording_set)
  int64_t rec_n = 0;
  // ohw_state_vad_frames: scratch of its own (staged host samples, band energies, probabilities, histogram + floor), grown on demand
  DevBuf vad_pcm, vad_e, vad_p, vad_aux;
  // recording slots (ohw_recording_set_slot / ohw_mel_seek_slots), nothing until a slot is first set: one recording per slot,
  // each buffer sized by the largest recording the state has seen when it was (re)allocated; slot_n: samples held (0: empty);
  // slot_max: i32 [max_batch] ordered-int maxima; slot_tab: the call's tables, [entries] each of offsets i64, pointers,
  // lengths i64, maximum indices i32
  std::vector<DevBuf> slot_pcm;
  std::vector<int64_t> slot_n;
  int64_t slot_cap = 0, slot_tab_entries = 0;
  DevBuf slot_max, slot_tab;
  // encoder activations
  DevBuf c1, h, y, qkv, att, ffn, enc;
  // taps kept for diagnostics (small models / tests only)
  DevBuf tap_stem, tap_block0;
  bool taps = false;
  // decoder
  DevBuf xkv;      // T [2L][B][H][1500][64]
  DevBuf self_kv;  // T [L][2][B][H][n_text_ctx][64]
  DevBuf dx, dy, dq, da, df, logits;
  DevBuf dln;                   // the LayerNorm of a step's rows, 16-bit tiles: scratch of the all-rows LN1 + QKV / LN2 + mlp.0 forms (decode.hip)
  DevBuf dx16, xstat;            // post-norm path: 16-bit tiled copy of the residual stream, per-16-column statistics
  bool postnorm = true;
  DevBuf ks_slab, ks_ticket;   // split-K partial tiles and arrival tickets of the decoder's RESID GEMMs
  int ksplit_long = 1, ksplit_short = 1;
  int stream_cus = 0;            // CUs of the current stream's mask (0 = unrestricted)
  bool skip_done = false;        // inside ohw_greedy: cross-attention skips windows whose done flag is set
  DevBuf samp_part, samp_ticket;   // sampler: per-slice partial states and arrival tickets
  DevBuf samp_temp, samp_u;        // the temperature sampler's T [1] and pre-drawn canonical doubles [B][max_tokens] (ohw_sample_pass)
  DevBuf xa_part, xa_ticket;       // cross-attention over key slices (small batches)
  int xa_rows = 0;
  DevBuf step_tok, n_past, tokens, n_cur, next_tok, done, n_done, sum_lp;
  // beam search (made on first use): candidates, cumulative scores, the kv_slot / token-history double buffers, finished pool
  DevBuf bm_cand_lp, bm_cand_tok, bm_sum, bm_slot[2], bm_tok2, bm_ncur, bm_npast, bm_done, bm_fin_cnt, bm_fin_tok, bm_fin_len, bm_fin_sum, bm_part, bm_ticket;
  // ohw_beam_search_ex only (made on its first use): per-token log-probability histories (double buffer, pool), the device-side
  // ranking's result rows
  DevBuf bm_plog[2], bm_fin_plog, bm_out_tok, bm_out_lp, bm_out_n, bm_out_sum, bm_out_eot, bm_out_nfin, bm_nosp;
  // the captured iterations (GraphCache), a handful each.  step_graphs: one greedy or temperature iteration {feed the sampled
  // token, single-token decoder step, sampler} per (batch, ...) seen; group_graphs: best-of sampling's {decoder step with
  // kv_group = N, group sampler}, keyed on N as well and kept apart from step_graphs; beam_graphs: the odd and the even beam
  // iteration of a (windows, beam size, ...) key as one entry, so a call never holds an exec of an entry it then evicts
  GraphCache step_graphs{8}, group_graphs{4}, beam_graphs{4, true};
  // the persistent small-batch decoder step (decode_persist.hip): per-layer pointer table, granule arena, epoch / abort words
  DevBuf ps_layers, ps_gran, ps_words;
  PersistParams ps_layout{};         // region offsets of the arena
  bool persist = false;              // OHW_DEC_PERSIST / ohw_state_set_persistent (off: measured slower than the launches)
  bool fuse_attn = false;            // OHW_DEC_FUSE_ATTN=1: small single-token steps run their self-attention inside the QKV launch (measured slower: off)
  DevBuf attn_ticket;                // u32 [n_text_head], zero between launches
  int persist_launches = 0;
  int n_cu = 0;
  // which decoder kernel instantiations run_decoder_step launched (ohw_dbg_counter "dec_gemm.*", "xattn.*", "self_attn.*"):
  // counted on the host, so a captured step counts once, at its capture
  int64_t tally_gemm[DT_GEMMS][DT_FORMS][DG_N_SHAPES] = {};
  int64_t tally_xattn[XA_N_VARIANTS] = {};
  int64_t tally_self[4] = {};      // SA_PLAIN, SA_SLOTS, then the same two run inside the QKV launch (OHW_DEC_FUSE_ATTN)
  DevBuf tok_lp, nosp_prob;        // per-token log-probabilities [B][max_tokens + 1], no-speech probability [B]
  LogitRules rules;                // logit bias, hot phrases, repetition rule, command list: logit_rules.hpp owns them and their order
  int m_max = 0;
  int64_t logits_ld = 0;
  // per-kernel-class profiling (bench): event pairs around every launch of one class
  int prof_class = 0;
  std::vector<hipEvent_t> prof_ev;
  size_t prof_used = 0;
  double prof_work = 0.0;
  bool batch_invariant = false;      // cross-attention variant picked from n_new alone (state_set_batch_invariant)
  // best-of sampling (ohw_sample_pass_n; made on first use): the pass's constant kv_slot table [rows][n_text_ctx], then per window
  // {shared length, active, done flag, finished-row count} [4][max_batch]; sn_rows: rows of the last pass's table ("sample_slots")
  DevBuf sn_slot, sn_win;
  int sn_rows = 0;
  bool graphs_enabled = true;
  int graph_max_batch = 32;         // graphs for batches below this (OHW_GRAPH_MAX_BATCH)
  // word timestamps (ohw_state_set_align_heads / ohw_state_align; align.hip).  al_heads: the caller's list; the buffers are made
  // when a list is set.  al_rows = n_text_ctx / 2 + 8 token rows per (window, head).  al_tap is set only while ohw_state_align
  // replays a window's tokens: run_decoder_step then taps the listed heads behind each layer's cross-query GEMM, row al_row0 on.
  // al_nall / al_nk / al_prompt / al_batch describe the last alignment (ohw_state_fetch "align_*")
  std::vector<ohw_align_head> al_heads;
  DevBuf al_p, al_q, al_stats, al_m, al_trace, al_idx, al_cnt, al_tok;   // al_cnt i32 [3][max_batch]: n_all, n_keys, N
  int al_rows = 0;
  bool al_tap = false;
  int al_row0 = 0, al_lds = 0;
  std::vector<int32_t> al_nall, al_nk;
  int al_prompt = 0, al_batch = 0;
  // confidence (ohw_state_score; score.hip), nothing until the first scoring call or ohw_state_set_score_buffers.  sc_logits: the
  // all-rows logits of ONE replay chunk, f32 [max_batch * 8][logits_ld]; sc_tok / sc_tgt: the chunks' tokens and targets,
  // [chunk][batch][8]; sc_cnt i32 [max_batch]: positions with a score; sc_out: ohw_token_score [max_batch][n_text_ctx / 2 + 1].
  // sc_on is set only while ohw_state_score replays: run_decoder_step's logits GEMM then stores every row to sc_logits.
  // sc_keep (ohw_state_set_score_buffers(st, 2)): the rows of the call's last window, every chunk, for the "score_logits" fetch;
  // sc_batch / sc_chunks / sc_kept describe them
  DevBuf sc_logits, sc_tok, sc_tgt, sc_cnt, sc_out, sc_keep;
  bool sc_on = false, sc_keep_rows = false;
  int sc_batch = 0, sc_chunks = 0;
  int64_t tally_score = 0;           // token_score_kernel launches (ohw_dbg_counter "token_score")
  // timing
  hipEvent_t ev[6]{};
  ohw_timings last{};
  int max_tokens = 0;
};

template <typename F>
const GraphEntry& GraphCache::get_or_capture(ohw_state* st, const GraphKey& key, int n_graphs, F&& body) {
  if (const GraphEntry* e = find(key)) return *e;
  // room first: the oldest entry goes before anything of this call exists (an eviction between the two captures of a pair
  // once dropped an entry whose exec the call might already hold)
  if (entries.size() >= capacity) {
    entries.front().destroy();
    entries.erase(entries.begin());
  }
  GraphEntry ng;
  ng.key = key;
  try {
    for (int q = 0; q < n_graphs; ++q) {
      // The iteration is captured on the state's OWN stream (non-blocking) and replayed on whatever stream the state
      // runs on: a CU-masked stream (hipExtStreamCreateWithCUMask) is a blocking stream, and while a blocking stream
      // captures, any use of the legacy stream by another thread - another engine loading its model, say - fails with
      // "would make the legacy stream depend on a capturing blocking stream" and kills the capture (two engines driven
      // by two threads: tests/test_gpu_configs.py).  The own stream is idle whenever the state runs on an external one.
      // Capture mode RELAXED: in the other modes HIP (ROCm 7.2) rejects every synchronous memory call of EVERY thread
      // while a capture is open - hipMemset in another engine's state allocation failed that way - and this thread
      // makes no call during the capture that the stricter modes would have to catch.
      hipStream_t cap = st->own_stream;
      CaptureGate gate;   // no other thread is inside the library while this stream captures (common.hpp)
      struct StreamSwap { ohw_state* st; hipStream_t keep; ~StreamSwap() { st->stream = keep; } } swap{st, st->stream};
      st->stream = cap;
      if (marks) BMARK("capture begin", q);
      HIP_CHECK(hipStreamBeginCapture(cap, hipStreamCaptureModeRelaxed));
      try {
        body(q, cap);
      } catch (...) {
        hipGraph_t g = nullptr;
        (void)hipStreamEndCapture(cap, &g);
        if (g) (void)hipGraphDestroy(g);
        throw;
      }
      HIP_CHECK(hipStreamEndCapture(cap, &ng.graph[q]));
      if (marks) BMARK("capture ended", q);
      HIP_CHECK(hipGraphInstantiate(&ng.exec[q], ng.graph[q], nullptr, nullptr, 0));
      if (marks) BMARK("instantiated", q);
    }
  } catch (...) {
    ng.destroy();     // a partially built entry goes whole; only a complete one is kept
    throw;
  }
  entries.push_back(ng);
  ++captures;
  return entries.back();
}

namespace {

// the key of an iteration captured now: the state's settings that the captured launches bake in, and the caller's own terms
GraphKey graph_key(const ohw_state* st, int rows, int group, bool flag, const SamplerParams& spar) {
  GraphKey k;
  k.rows = rows; k.group = group; k.cus = st->stream_cus; k.t_len = st->enc_ctx; k.var = st->enc_var; k.invariant = st->batch_invariant;
  k.persist = st->persist; k.flag = flag; k.phrases = st->rules.ph.on; k.repeat = st->rules.rp.on; k.commands = st->rules.cm.on;
  std::memcpy(&k.spar, &spar, sizeof spar);
  return k;
}

// while one lives (and is on), cross-attention skips the windows whose done flag is set; the earlier setting returns after it
struct SkipDone {
  bool& f;
  bool keep;
  explicit SkipDone(bool& r, bool on = true) : f(r), keep(r) { if (on) f = true; }
  ~SkipDone() { f = keep; }
};

struct ProfScope {
  ohw_state* st;
  bool on;
  ProfScope(ohw_state* s, int cls, double work) : st(s), on(s->prof_class == cls) {
    if (!on) return;
    if (st->prof_used + 2 > st->prof_ev.size()) {
      const size_t old = st->prof_ev.size();
      st->prof_ev.resize(old + 1024);
      for (size_t i = old; i < st->prof_ev.size(); ++i) HIP_CHECK(hipEventCreateWithFlags(&st->prof_ev[i], hipEventDisableSystemFence));
    }
    HIP_CHECK(hipEventRecord(st->prof_ev[st->prof_used], st->stream));
    st->prof_work += work;
  }
  ~ProfScope() {
    if (!on) return;
    (void)hipEventRecord(st->prof_ev[st->prof_used + 1], st->stream);
    st->prof_used += 2;
  }
};

struct Dispatch {
  template <typename F> static void run(int dtype, F&& f) {
    if (dtype == OHW_DTYPE_BF16) f((bf16_t*)nullptr);
    else f((f16_t*)nullptr);
  }
};

void persist_prepare(ohw_state* st);

// encoder positions per window in effect (ohw_state_set_audio_ctx)
int audio_ctx_of(const ohw_state* st) { return st->audio_ctx > 0 ? st->audio_ctx : st->ctx->hp.n_audio_ctx; }
void check_decode_ctx(const ohw_state* st, const char* what) {
  if (audio_ctx_of(st) != st->enc_ctx)
    throw Error(OHW_E_INVALID_ARG, std::string(what) + ": the audio context changed since the last ohw_encode (" + std::to_string(st->enc_ctx) + " -> " +
                                       std::to_string(audio_ctx_of(st)) + "): encode again");
  if (st->win_ctx != st->enc_set)
    throw Error(OHW_E_INVALID_ARG, std::string(what) + ": the per-window contexts changed since the last ohw_encode: encode again");
}
// a decode under a language table (ohw_state_set_window_lang): the table names exactly the decode batch and nothing waits
void check_window_lang(const ohw_state* st, int windows, const std::string& what) {
  if ((int)st->lang_kind.size() != windows)
    throw Error(OHW_E_INVALID_ARG, what + ": ohw_state_set_window_lang named " + std::to_string(st->lang_kind.size()) + " windows, the decode batch has " +
                                       std::to_string(windows));
  for (int b = 0; b < windows; ++b)
    if (st->lang_kind[(size_t)b] == ohw_state::LANG_WAITING)
      throw Error(OHW_E_INVALID_ARG, what + ": window " + std::to_string(b) + "'s language is still to be detected: call ohw_state_detect_window_lang first");
}
// a new encode: what was detected belonged to the old audio and waits again; explicit entries stay
void window_lang_after_encode(ohw_state* st) {
  bool any = false;
  for (auto& k : st->lang_kind)
    if (k == ohw_state::LANG_RESOLVED) { k = ohw_state::LANG_WAITING; any = true; }
  if (!any) return;
  HIP_CHECK(hipMemcpyAsync(st->lang_tab.p, st->lang_ids.data(), st->lang_ids.size() * 4, hipMemcpyHostToDevice, st->stream));
  HIP_CHECK(hipStreamSynchronize(st->stream));     // pageable source
}
// the mel pass under the state's per-window contexts: they must name exactly its windows
const int32_t* mel_win_ctx(ohw_state* st, int batch) {
  if (st->win_ctx.empty()) return nullptr;
  if ((int)st->win_ctx.size() != batch)
    throw Error(OHW_E_INVALID_ARG, "mel: ohw_state_set_window_ctx named " + std::to_string(st->win_ctx.size()) + " windows, the call has " + std::to_string(batch));
  return st->wc_enc.as<int32_t>();
}

void state_alloc(ohw_state* st) {
  const ohw_ctx* c = st->ctx;
  const ohw_hparams& hp = c->hp;
  const int64_t B = st->max_batch, d = hp.n_audio_state, dt = hp.n_text_state, T = hp.n_audio_ctx;
  const int64_t L = hp.n_text_layer, H = hp.n_text_head;
  st->pcm.alloc((size_t)B * CHUNK_SAMPLES * 4);
  st->n_samples.alloc((size_t)B * 4);
  st->logmel.alloc((size_t)B * hp.n_mels * CHUNK_FRAMES * 4);
  st->max_bits.alloc((size_t)B * 4);
  st->mel_t.alloc((size_t)B * MEL_ROWS * MEL_CPAD * 2, true);
  st->c1.alloc((size_t)B * MEL_ROWS * d * 2 + 4 * d * 2, true);  // + slack: the last conv2 row reads 1 row past
  st->h.alloc((size_t)B * T * d * 4);
  st->y.alloc((size_t)B * T * d * 2);
  st->qkv.alloc((size_t)B * T * 3 * d * 2);
  st->att.alloc((size_t)B * T * d * 2);
  st->ffn.alloc((size_t)B * T * 4 * d * 2);
  st->enc.alloc((size_t)B * T * d * 2);
  st->taps = d <= 512;
  if (st->taps) {
    st->tap_stem.alloc((size_t)B * T * d * 4);
    st->tap_block0.alloc((size_t)B * T * d * 4);
  }
  st->xkv.alloc((size_t)2 * L * B * H * T * 64 * 2);
  st->self_kv.alloc((size_t)L * 2 * B * H * hp.n_text_ctx * 64 * 2, true);
  st->m_max = (int)B * 16;      // a 16-position prefill chunk of every window; the decode entries keep to 8 tokens per window
  st->dx.alloc((size_t)st->m_max * dt * 4);
  // dy / da / df are read as 16-row activation tiles by 32-row workgroups: whole tiles, zeroed once (rows past M are
  // multiplied but never stored)
  const size_t m_tiles = ((size_t)st->m_max + 31) / 32 * 32;
  st->dy.alloc(m_tiles * dt * 2, true);
  st->dln.alloc(m_tiles * dt * 2, true);
  // post-norm decoder GEMMs (decode.hip): OHW_DEC_POSTNORM=1 (off by default: measured, no gain - the LayerNorm prologue
  // already hides under the weights' first-byte latency); never with a split-K knob (the split path
  // publishes no statistics); dt must be a multiple of 32
  st->graphs_enabled = env_int("OHW_GRAPHS", 1, 0, 1) != 0;      // 0: the decode iterations are launched kernel by kernel (diagnostics)
  // the greedy iteration is replayed as a hipGraph below this batch size only: a graph pays while the step is launch-bound
  // (one window: 260 launches of 3 - 6 us); from 32 windows on a step's kernels outlast their launches (measured equal,
  // 371.0 ms per 32-window batch either way) and in the LANES schedule the replayed graphs lose 2.4 % to sporadic 40-us
  // stalls inside a replay (tools/lane_gap_analysis.py) - and a lane's first call no longer waits, at its capture, for the
  // other lanes to leave the library
  st->graph_max_batch = env_int("OHW_GRAPH_MAX_BATCH", 32, 1, 1 << 20);
  st->persist = env_int("OHW_DEC_PERSIST", 0, 0, 1) != 0;
  st->fuse_attn = env_int("OHW_DEC_FUSE_ATTN", 0, 0, 1) != 0;
  st->gemm_small = env_int("OHW_GEMM_SMALL", 0, 0, 1) != 0;
  st->packed = env_int("OHW_ENC_PACKED", 0, 0, 1) != 0;
  st->pk_off.alloc((size_t)(B + 1) * 4, true);
  st->pk_map.alloc((size_t)B * T * 4, true);
  st->mel_ctx = st->enc_ctx = hp.n_audio_ctx;
  st->wc_enc.alloc((size_t)B * 4, true);
  st->wc_dec.alloc((size_t)B * 4, true);
  st->enc_win.assign((size_t)B, 0);
  st->lang_tab.alloc((size_t)B * 4, true);
  st->lang_prob.alloc((size_t)B * std::max(1, c->tok.n_langs) * 4, true);
  st->attn_ticket.alloc((size_t)hp.n_text_head * 4, true);
  st->wp_chunks = (hp.n_text_ctx / 2 + 7) / 8;
  st->wp_feed.alloc((size_t)((hp.n_text_ctx / 2 + 15) / 16) * 16 * B * 4, true);      // whole chunks of either size
  st->wp_pos.alloc((size_t)st->wp_chunks * B * 4, true);
  st->wp_done.alloc((size_t)st->wp_chunks * B * 4, true);
  st->wp_lens.alloc((size_t)B * 4, true);
  st->prefill_xa = env_int("OHW_PREFILL_XA", 1, 0, 1) != 0;
  (void)hipDeviceGetAttribute(&st->n_cu, hipDeviceAttributeMultiprocessorCount, c->device);
  st->postnorm = env_int("OHW_DEC_POSTNORM", 0, 0, 1) != 0 && dec_ksplit_long() == 1 && dec_ksplit_short() == 1 && dt % 32 == 0;
  st->dx16.alloc(m_tiles * dt * 2, true);
  st->xstat.alloc((size_t)st->m_max * (dt / 16) * 2 * 4, true);
  st->dq.alloc((size_t)st->m_max * dt * 2);
  st->da.alloc(m_tiles * dt * 2, true);
  st->df.alloc(m_tiles * 4 * dt * 2, true);
  {
    const size_t tiles = (size_t)((dt + 15) / 16) * ((st->m_max + 31) / 32);
    st->ks_slab.alloc(tiles * DEC_KSPLIT_MAX * 2048);
    st->ks_ticket.alloc(tiles * 4, true);
    st->samp_part.alloc((size_t)B * SAMPLER_SPLIT * SAMPLER_PART_WORDS * 4, true);
    st->samp_ticket.alloc((size_t)B * 4, true);
    st->xa_rows = std::min(st->m_max, 24);       // 24 rows x 20 heads is already two (row, head) pairs per CU
    st->xa_part.alloc((size_t)st->xa_rows * H * XA_MAX_SPLIT * 68 * 4, true);
    st->xa_ticket.alloc((size_t)st->xa_rows * H * 4, true);
    st->ksplit_long = dec_ksplit_long();
    st->ksplit_short = dec_ksplit_short();
  }
  st->logits_ld = c->v_pad;
  st->logits.alloc((size_t)B * st->logits_ld * 4);
  st->max_tokens = hp.n_text_ctx;
  st->step_tok.alloc((size_t)st->m_max * 4);
  st->n_past.alloc((size_t)B * 4, true);
  st->tokens.alloc((size_t)B * st->max_tokens * 4, true);
  st->n_cur.alloc((size_t)B * 4, true);
  st->next_tok.alloc((size_t)B * 4, true);
  st->done.alloc((size_t)B * 4, true);
  st->n_done.alloc(16, true);
  st->sum_lp.alloc((size_t)B * 4, true);
  st->tok_lp.alloc((size_t)B * (st->max_tokens + 1) * 4, true);
  st->nosp_prob.alloc((size_t)B * 4, true);
  st->samp_temp.alloc(16, true);
  st->samp_u.alloc((size_t)B * st->max_tokens * 8, true);
  for (auto& e : st->ev) HIP_CHECK(hipEventCreate(&e));
  persist_prepare(st);
}

// the persistent decoder step's granule arena, epoch / abort words and per-layer pointer table (decode_persist.hip): made with
// the state, never lazily - a first use inside a graph capture must not allocate or memset
bool persist_dims_ok(const ohw_hparams& hp) {
  return hp.n_text_state % 64 == 0 && hp.n_text_state <= 1280 && hp.n_text_head * 64 == hp.n_text_state;
}
void persist_prepare(ohw_state* st) {
  const ohw_ctx* c = st->ctx;
  const ohw_hparams& hp = c->hp;
  if (!persist_dims_ok(hp) || st->ps_gran.p) return;
  PersistParams q{};
  q.d = hp.n_text_state; q.H = hp.n_text_head;
  const int64_t n_gran = persist_layout(&q);
  st->ps_gran.alloc((size_t)n_gran * 8, true);
  st->ps_words.alloc(64, true);
  const unsigned one = 1;
  HIP_CHECK(hipMemcpy(st->ps_words.p, &one, 4, hipMemcpyHostToDevice));
  std::vector<PersistLayer> lw((size_t)hp.n_text_layer);
  for (int l = 0; l < hp.n_text_layer; ++l) {
    const DecLayerW& w = c->dec[l];
    lw[(size_t)l] = PersistLayer{w.wqkv.p, w.wo.p, w.wxq.p, w.wxo.p, w.w1.p, w.w2.p, w.bqkv.as<float>(), w.bo.as<float>(), w.bxq.as<float>(),
                                 w.bxo.as<float>(), w.b1.as<float>(), w.b2.as<float>()};
  }
  st->ps_layers.alloc(lw.size() * sizeof(PersistLayer));
  HIP_CHECK(hipMemcpy(st->ps_layers.p, lw.data(), lw.size() * sizeof(PersistLayer), hipMemcpyHostToDevice));
  st->ps_layout = q;
}

template <typename T>
void run_mel(ohw_state* st, const float* pcm_dev, int64_t stride, int batch, int mode) {
  const ohw_ctx* c = st->ctx;
  MelParams p{};
  p.pcm = pcm_dev; p.pcm_stride = stride; p.n_samples = st->n_samples.as<int32_t>();
  p.filters = c->mel_filters.as<float>(); p.twiddle = c->twiddle.as<float>(); p.window = c->window.as<float>();
  p.logmel = st->logmel.as<float>(); p.max_bits = st->max_bits.as<int32_t>(); p.mel_t = st->mel_t.p;
  p.n_mels = c->hp.n_mels; p.batch = batch; p.mode = mode;
  p.frame_limit = 2 * audio_ctx_of(st);
  p.win_ctx = mel_win_ctx(st, batch);
  launch_mel<T>(p, st->stream);
  st->mel_ctx = audio_ctx_of(st);
  st->mel_win = st->win_ctx;
}

// first / total: the cross K/V of these B windows go to windows [first, first + B) of a decode batch of `total` windows
template <typename T>
void run_encode(ohw_state* st, int B, int first, int total) {
  const ohw_ctx* c = st->ctx;
  const ohw_hparams& hp = c->hp;
  hipStream_t s = st->stream;
  // Tn: encoder positions per window - the state's audio context; conv1 runs the 2 * Tn frames conv2 reads (image row
  // 1 + 2 * Tn, conv1's right padding, was written as zeros by the mel pass)
  const int64_t d = hp.n_audio_state, Tn = audio_ctx_of(st), M = (int64_t)B * Tn;
  // a short window: the 64x64-tile kernel where the 128x128 grid would leave more than half the compute units idle
  const bool reduced = Tn < hp.n_audio_ctx;
  // per-window contexts: every buffer keeps the envelope's strides, the GEMMs and LayerNorms run all B * Tn rows (rows past a
  // window's length hold unspecified values no valid row reads), the attention - the part that is quadratic in the length -
  // runs each window at its own length
  const bool var = !st->win_ctx.empty();
  double attn_sq = (double)B * (double)Tn * (double)Tn;     // sum over the windows of (queries x keys)
  int64_t Mp = 0;                                           // sum of the lengths
  bool ragged = false;
  if (var) {
    attn_sq = 0.0;
    for (int b = 0; b < B; ++b) {
      attn_sq += (double)st->win_ctx[(size_t)b] * (double)st->win_ctx[(size_t)b];
      Mp += st->win_ctx[(size_t)b];
      ragged = ragged || st->win_ctx[(size_t)b] != Tn;
    }
  }
  // packed rows (ohw_state_set_packed_encoder): behind the conv stem the windows lie end to end - row
  // pk_off[b] + t of h, y, qkv, att, ffn, enc and the block0 tap is position t of window b - so the LayerNorms and the dense GEMMs
  // (row-wise, hence the same bits per row) run Mp rows instead of B * Tn; the attention finds its window at pk_off[b], the
  // cross-K/V GEMM scatters its rows to the unpacked [2L][B][H][Tn][64] through pk_map.  Lengths that all equal the envelope
  // are the uniform layout already: the path as it stands
  const bool packed = var && st->packed && ragged;
  const int64_t Md = packed ? Mp : M;                       // rows of the dense stages
  st->enc_rows = Md;
  st->enc_pk.clear();
  if (packed) {
    int64_t o = 0;
    for (int b = 0; b < B; ++b) { st->enc_pk.push_back(o); o += st->win_ctx[(size_t)b]; }
    launch_pack_map(st->wc_enc.as<int32_t>(), B, (int)Tn, st->pk_off.as<int32_t>(), st->pk_map.as<int32_t>(), s);
  }
  auto pick_small = [&](GemmParams& q) {
    const int64_t tiles128 = ((q.M + 127) / 128) * (q.N / 128);
    q.small_m = reduced && st->gemm_small && q.N % 64 == 0 && q.K % 64 == 0 && 2 * tiles128 < (st->n_cu > 0 ? st->n_cu : 256) ? 1 : 0;
  };
  GemmParams g{};
  // conv1 (k=3, pad 1) as a GEMM over overlapping rows of the time-major mel image
  g = GemmParams{};
  g.A = st->mel_t.p; g.W = c->conv1_w.p; g.bias = c->conv1_b.as<float>();
  g.out = (T*)st->c1.p + d;  // output row t -> image row 1 + t
  g.M = (int64_t)B * 2 * Tn; g.N = d; g.K = 3 * MEL_CPAD;
  g.lda = MEL_CPAD; g.a_batch_stride = (int64_t)MEL_ROWS * MEL_CPAD; g.rows_per_batch = 2 * Tn;
  g.ldc = d; g.c_batch_stride = (int64_t)MEL_ROWS * d;
  pick_small(g);
  { ProfScope ps(st, OHW_PROF_ENC_GEMM, 2.0 * g.M * g.N * g.K); launch_gemm<T>(g, EPI_BIAS_GELU_T, s); }
  // conv2 (k=3, stride 2, pad 1): row t reads image rows 2t .. 2t+2 of conv1's padded output
  g = GemmParams{};
  g.A = st->c1.p; g.W = c->conv2_w.p; g.bias = c->conv2_b.as<float>(); g.pos = c->enc_pos.as<float>();
  // packed: conv2 writes its B * Tn rows into the ffn buffer (idle until block 0's mlp, and B * Tn * 4d 16-bit elements hold
  // B * Tn * d floats twice over), the pack kernel gathers the valid ones from there into h: a second buffer, not an ordered copy
  g.out = packed ? st->ffn.p : st->h.p;
  g.M = M; g.N = d; g.K = 3 * d;
  g.lda = 2 * d; g.a_batch_stride = (int64_t)MEL_ROWS * d; g.rows_per_batch = Tn;
  g.ldc = d; g.c_batch_stride = Tn * d;
  pick_small(g);
  { ProfScope ps(st, OHW_PROF_ENC_GEMM, 2.0 * g.M * g.N * g.K); launch_gemm<T>(g, EPI_GELU_POS_F32, s); }
  if (st->taps) HIP_CHECK(hipMemcpyAsync(st->tap_stem.p, g.out, (size_t)M * d * 4, hipMemcpyDeviceToDevice, s));
  if (packed) launch_pack_rows(st->ffn.as<float>(), st->pk_map.as<int32_t>(), st->h.as<float>(), Md, (int)d, s);

  auto dense = [&](const void* A, int64_t K, const DevBuf& W, const DevBuf& bias, void* out, int64_t N, int epi) {
    GemmParams q{};
    q.A = A; q.W = W.p; q.bias = bias.as<float>(); q.out = out;
    q.M = Md; q.N = N; q.K = K; q.lda = K; q.a_batch_stride = 0; q.rows_per_batch = Md; q.ldc = N; q.c_batch_stride = 0;
    pick_small(q);
    ProfScope ps(st, OHW_PROF_ENC_GEMM, 2.0 * q.M * q.N * q.K);
    launch_gemm<T>(q, epi, s);
  };
  for (int l = 0; l < hp.n_audio_layer; ++l) {
    const EncLayerW& w = c->enc[l];
    launch_layernorm<T>(st->h.as<float>(), w.ln1.g.as<float>(), w.ln1.b.as<float>(), st->y.p, Md, (int)d, s);
    dense(st->y.p, d, w.wqkv, w.bqkv, st->qkv.p, 3 * d, EPI_BIAS_T);
    {
      ProfScope ps(st, OHW_PROF_ENC_ATTN, 4.0 * hp.n_audio_head * attn_sq * 64.0);
      launch_encoder_attention<T>(st->qkv.p, st->att.p, B, (int)Tn, hp.n_audio_head, s, var ? st->wc_enc.as<int32_t>() : nullptr,
                                  packed ? st->pk_off.as<int32_t>() : nullptr);
    }
    dense(st->att.p, d, w.wo, w.bo, st->h.p, d, EPI_BIAS_RESID_F32);
    launch_layernorm<T>(st->h.as<float>(), w.ln2.g.as<float>(), w.ln2.b.as<float>(), st->y.p, Md, (int)d, s);
    dense(st->y.p, d, w.w1, w.b1, st->ffn.p, 4 * d, EPI_BIAS_GELU_T);
    dense(st->ffn.p, 4 * d, w.w2, w.b2, st->h.p, d, EPI_BIAS_RESID_F32);
    if (l == 0 && st->taps) HIP_CHECK(hipMemcpyAsync(st->tap_block0.p, st->h.p, (size_t)Md * d * 4, hipMemcpyDeviceToDevice, s));
  }
  launch_layernorm<T>(st->h.as<float>(), c->ln_post.g.as<float>(), c->ln_post.b.as<float>(), st->enc.p, Md, (int)d, s);
  // cross-attention K/V of every decoder layer in one GEMM: N = 2 * L * d, head-major output
  g = GemmParams{};
  g.A = st->enc.p; g.W = c->xkv_w.p; g.bias = c->xkv_b.as<float>(); g.out = st->xkv.p;
  g.M = M; g.N = (int64_t)2 * hp.n_text_layer * hp.n_text_state; g.K = d;
  g.lda = d; g.a_batch_stride = Tn * d; g.rows_per_batch = Tn; g.ldc = 0; g.c_batch_stride = 0;
  g.d_model = hp.n_text_state; g.n_head = hp.n_text_head; g.t_len = (int)Tn; g.batch = total; g.batch_offset = first;
  if (packed) {   // A packed and dense, every output row to its (window, position) of the unpacked slabs
    g.M = Md; g.a_batch_stride = 0; g.rows_per_batch = Md; g.c_row_map = st->pk_map.as<int32_t>();
  }
  pick_small(g);
  { ProfScope ps(st, OHW_PROF_ENC_GEMM, 2.0 * g.M * g.N * g.K); launch_gemm<T>(g, EPI_CROSSKV_T, s); }
  // the lengths of these windows into their decode-batch slots
  if (var) HIP_CHECK(hipMemcpyAsync(st->wc_dec.as<int32_t>() + first, st->wc_enc.p, (size_t)B * 4, hipMemcpyDeviceToDevice, s));
}

// one decoder pass over M = B * n_new rows; tokens in tok_src (default st->step_tok), positions from st->n_past
// kv_group > 1 (beam search): B rows are kv_group beams per window - cross K/V is per window, self K/V goes through kv_slot,
// win_done flags whole windows
// want_logits = false (the prefill's chunks): the pass ends behind the last layer - only the self K/V it leaves in the cache is wanted
// chunk_xa (the prefill's chunks, n_new = 8 or 16): cross-attention through cross_attn_chunk_kernel under the rule of the rows path
template <typename T>
void run_decoder_step(ohw_state* st, int B, int n_new, const int32_t* tok_src = nullptr, int kv_group = 1, const int32_t* kv_slot = nullptr,
                      const int32_t* win_done = nullptr, bool want_logits = true, bool chunk_xa = false) {
  const ohw_ctx* c = st->ctx;
  const ohw_hparams& hp = c->hp;
  hipStream_t s = st->stream;
  // Tn: keys per cross-attention = the context of the last encode (the entries refuse a call under another one)
  const int d = hp.n_text_state, H = hp.n_text_head, C = hp.n_text_ctx, Tn = st->enc_ctx, L = hp.n_text_layer;
  const int M = B * n_new;
  if (M > st->m_max) throw Error(OHW_E_INVALID_ARG, "decode: batch * n_new exceeds the state's capacity (16 tokens per window per call)");
  const int32_t* n_past = st->n_past.as<int32_t>();
  const bool pn = st->postnorm;
  // ---- at most 16 single-token rows: the 32 layers in ONE persistent launch (decode_persist.hip) instead of 8 launches per
  // layer.  Not under ohw_state_set_batch_invariant (a window's bits must then not depend on which path its batch takes), not
  // while a kernel class is being profiled, not on the experimental post-norm / split-K paths.
  const bool var = st->enc_var;   // per-window contexts: the launches below, the variant choice of batch-invariant mode
  if (st->persist && n_new == 1 && M <= 16 && kv_group <= 5 && M % kv_group == 0 && !st->batch_invariant && !var && !pn && st->prof_class == 0 &&
      st->ksplit_long == 1 && st->ksplit_short == 1 && st->ps_gran.p) {
    const int grid = std::max(1, std::min(st->stream_cus > 0 ? st->stream_cus : st->n_cu, 256));
    PersistParams q = st->ps_layout;
    launch_embed<T>(c->emb.p, c->dec_pos.as<float>(), tok_src ? tok_src : st->step_tok.as<int32_t>(), n_past, st->dx.as<float>(), nullptr, nullptr, M, 1, d, s);
    const int Wn = M / kv_group;
    q.layers = st->ps_layers.as<PersistLayer>(); q.L = L; q.M = M; q.group = kv_group; q.d = d; q.H = H; q.n_ctx = C; q.t_len = Tn;
    q.S = std::max(1, std::min(16, grid / std::max(1, Wn * H)));
    // a short context: no slice without an 8-key group (at 1500 keys, 188 groups, every S <= 16 already passes)
    for (const int ng = (Tn + 7) / 8; q.S > 1 && (q.S - 1) * ((ng + q.S - 1) / q.S) >= ng;) --q.S;
    const int kb_mlp = 4 * d / 32;
    int ns = std::max(1, std::min(4, (grid + d / 16 - 1) / (d / 16)));
    while (ns < 4 && (kb_mlp + ns - 1) / ns + 1 > 56) ++ns;
    while (ns > 1 && kb_mlp / ns < 1) --ns;
    q.nsplit = ns;
    q.n_past = n_past; q.kv_slot = kv_slot;
    q.done = kv_group > 1 ? win_done : (st->skip_done ? st->done.as<int32_t>() : nullptr);
    q.x_in = st->dx.as<float>(); q.x_out = st->dx.as<float>();
    q.self_kv = st->self_kv.p; q.kv_layer = (int64_t)st->max_batch * H * C * 64; q.kv_row = (int64_t)H * C * 64;
    if ((int64_t)st->max_batch * q.kv_row * 2 >= ((int64_t)1 << 32)) throw Error(OHW_E_INVALID_ARG, "persistent step: a layer's K cache exceeds 4 GiB");
    q.xkv = st->xkv.p; q.xkv_slab = (int64_t)Wn * H * Tn * 64;
    q.g = st->ps_gran.as<unsigned long long>();
    q.epoch = st->ps_words.as<unsigned>(); q.abort_word = st->ps_words.as<unsigned>() + 8;
    launch_persist_step<T>(q, grid, s);
    ++st->persist_launches;
    launch_layernorm<T>(st->dx.as<float>(), c->dec_ln.g.as<float>(), c->dec_ln.b.as<float>(), st->dy.p, M, d, s, true);
    DecGemmParams lp{};
    lp.x = st->dy.p; lp.w = c->emb.p; lp.bias = nullptr; lp.out = st->logits.p; lp.cu_budget = st->stream_cus;
    lp.M = M; lp.N = hp.n_vocab; lp.K = d; lp.n_new = 1; lp.ld_out = st->logits_ld; lp.n_past = n_past; lp.d_model = d; lp.n_head = H; lp.n_ctx = C;
    ++st->tally_gemm[DT_LOGITS][DT_PLAIN][launch_dec_gemm<T>(lp, DEPI_LOGITS, s)];
    return;
  }
  launch_embed<T>(c->emb.p, c->dec_pos.as<float>(), tok_src ? tok_src : st->step_tok.as<int32_t>(), n_past, st->dx.as<float>(),
                  pn ? st->dx16.p : nullptr, pn ? st->xstat.as<float>() : nullptr, M, n_new, d, s);
  const int64_t kv_layer = (int64_t)st->max_batch * H * C * 64;      // elements per K (or V) cache of one layer
  const int64_t xkv_slab = (int64_t)(B / kv_group) * H * Tn * 64;    // cross K/V slab (batch of the last encode)
  auto gemm = [&](int which, const void* x, const LayerNormW* ln, const DevBuf& w, const DevBuf& bias, void* out, int N, int K, int epi, int64_t ld,
                  const DevBuf* wsum = nullptr) {
    DecGemmParams p{};
    p.x = x; p.w = w.p; p.bias = bias.p ? bias.as<float>() : nullptr; p.out = out;
    p.ln = ln ? 1 : 0; p.ln_rows = st->dln.p;
    if (ln && pn && wsum) {       // post-norm: the 16-bit tiled residual copy in, LayerNorm applied in the epilogue
      p.x = st->dx16.p; p.ln = 0; p.pn = 1; p.n_stat = K / 16; p.stat_in = st->xstat.as<float>(); p.wsum = wsum->as<float>();
    }
    if (epi == DEPI_BIAS_RESID && pn && N == d) { p.x16_out = st->dx16.p; p.stat_out = st->xstat.as<float>(); }
    p.cu_budget = st->stream_cus;
    if (epi == DEPI_BIAS_RESID) {
      const int ks = K >= 2 * d ? st->ksplit_long : st->ksplit_short;
      if (ks > 1 && ks <= K / 32) {
        p.ksplit = ks; p.slab = st->ks_slab.as<float>(); p.slab_bytes = (int32_t)st->ks_slab.bytes; p.ticket = st->ks_ticket.as<unsigned>();
      }
    }
    p.M = M; p.N = N; p.K = K; p.n_new = n_new; p.ld_out = ld; p.n_past = n_past;
    p.d_model = d; p.n_head = H; p.n_ctx = C;
    if (epi == DEPI_LOGITS && st->sc_on) { p.out_all = st->sc_logits.as<float>(); p.ld_all = st->logits_ld; }   // ohw_state_score's replay
    const int cls = epi == DEPI_BIAS_T ? OHW_PROF_DEC_GEMM_XQ : epi == DEPI_BIAS_GELU_T ? OHW_PROF_DEC_GEMM_FC1
                  : epi == DEPI_LOGITS ? OHW_PROF_DEC_GEMM_LOGITS : OHW_PROF_DEC_GEMM;
    // algorithmic bytes: the weights once per launch (the m-blocks of a prompt pass share them through L2)
    ProfScope ps(st, cls, 2.0 * (double)N * K);
    const int form = p.ln ? DT_LN : p.pn ? DT_PN : p.ksplit > 1 ? DT_KSPLIT : DT_PLAIN;
    ++st->tally_gemm[which][form][launch_dec_gemm<T>(p, epi, s)];
  };
  // OHW_DEC_FUSE_ATTN=1: single-token steps of at most 16 rows run their self-attention inside the QKV launch (decode.hip,
  // self_attn_row<COH>): one launch less per layer, the same bits - and 1.6 us per layer SLOWER (large-v3, one row: 77.3 against
  // 74.9 ms per 48-step chunk): the drain of the write-through stores, the ticket and the loads from beyond L2 are three dependent
  // round trips, a kernel boundary plus the separate launch's first bytes two.  Off.
  const bool fuse_attn = st->fuse_attn && n_new == 1 && M <= 16 && !pn && d % 64 == 0 && kv_layer * 2 < ((int64_t)1 << 31) && st->attn_ticket.p;
  for (int l = 0; l < L; ++l) {
    const DecLayerW& w = c->dec[l];
    T* kc = (T*)st->self_kv.p + (int64_t)(2 * l) * kv_layer;
    T* vc = kc + kv_layer;
    {  // LN1 + fused QKV projection; K/V go straight into the cache at each window's position
      DecGemmParams p{};
      p.x = st->dx.p; p.ln = 1; p.ln_rows = st->dln.p; p.cu_budget = st->stream_cus;
      if (pn) { p.x = st->dx16.p; p.ln = 0; p.pn = 1; p.n_stat = d / 16; p.stat_in = st->xstat.as<float>(); p.wsum = w.sqkv.as<float>(); }
      p.w = w.wqkv.p; p.bias = w.bqkv.as<float>(); p.out = st->dq.p;
      p.M = M; p.N = 3 * d; p.K = d; p.n_new = n_new; p.ld_out = d;
      p.k_cache = kc; p.v_cache = vc; p.n_past = n_past; p.d_model = d; p.n_head = H; p.n_ctx = C;
      if (fuse_attn) { p.attn_ticket = st->attn_ticket.as<unsigned>(); p.attn_out = st->da.p; p.attn_slots = kv_slot; p.kv_bytes = kv_layer * 2; }
      ProfScope ps(st, OHW_PROF_DEC_GEMM_QKV, 2.0 * (3.0 * d * d));
      ++st->tally_gemm[DT_QKV][p.pn ? DT_PN : DT_LN][launch_dec_gemm<T>(p, DEPI_QKV, s)];
    }
    if (!fuse_attn) ++st->tally_self[launch_self_attn<T>(st->dq.p, kc, vc, n_past, st->da.p, M, n_new, H, C, s, kv_slot)];
    else ++st->tally_self[2 + (kv_slot ? SA_SLOTS : SA_PLAIN)];
    gemm(DT_O, st->da.p, nullptr, w.wo, w.bo, st->dx.p, d, d, DEPI_BIAS_RESID, d);
    gemm(DT_XQ, st->dx.p, &w.lnx, w.wxq, w.bxq, st->dq.p, d, d, DEPI_BIAS_T, d, &w.sxq);
    if (st->al_tap) {     // ohw_state_align's replay: the listed heads of this layer read the queries just written and the layer's K
      AlignTapList list{};
      for (size_t a = 0; a < st->al_heads.size(); ++a)
        if (st->al_heads[a].layer == l) { list.slot[list.n] = (int16_t)a; list.head[list.n] = (int16_t)st->al_heads[a].head; ++list.n; }
      if (list.n > 0) {
        const int A = (int)st->al_heads.size();
        AlignTapParams tp{};
        tp.q = st->dq.p; tp.xk = (const T*)st->xkv.p + (int64_t)(2 * l) * xkv_slab; tp.n_head = H; tp.t_len = Tn;
        tp.rows = n_new; tp.row0 = st->al_row0; tp.row_cap = st->al_rows; tp.lds_stride = st->al_lds;
        tp.n_all = st->al_cnt.as<int32_t>(); tp.n_keys = st->al_cnt.as<int32_t>() + st->max_batch;
        tp.p = st->al_p.as<float>(); tp.p_row = hp.n_audio_ctx; tp.p_head = (int64_t)st->al_rows * tp.p_row; tp.p_win = (int64_t)A * tp.p_head;
        tp.p_fill = Tn; tp.q_out = st->al_q.as<float>(); tp.n_slots = A;
        launch_align_tap<T>(tp, list, B, s);
      }
    }
    {
      // algorithmic bytes: K and V of every (query row, head); the prompt pass streams them once per (window, head)
      // for all its rows (cross_attn_rows_kernel: same condition as launch_cross_attn)
      const bool chunk_path = chunk_xa && st->prefill_xa && (n_new == 8 || n_new == 16) && kv_group == 1 && ((int64_t)B * H >= 256 || st->batch_invariant || var);
      const bool rows_path = chunk_path || (n_new >= 2 && n_new <= 4 && ((int64_t)B * H >= 256 || st->batch_invariant || var));
      // (window, head) streams x keys: under per-window contexts the sum of the windows' own lengths
      double xa_keys = (double)(kv_group > 1 ? B / kv_group : rows_path ? B : M) * Tn;
      if (var) {
        xa_keys = 0.0;
        const int Wn = B / kv_group;
        for (int w = 0; w < Wn; ++w) xa_keys += (double)st->enc_win[(size_t)w] * (kv_group > 1 || rows_path ? 1 : n_new);
      }
      ProfScope psx(st, OHW_PROF_DEC_XATTN, 2.0 * 2.0 * xa_keys * H * 64.0);
      if (chunk_path) {
        launch_cross_attn_chunk<T>(st->dq.p, (const T*)st->xkv.p + (int64_t)(2 * l) * xkv_slab, (const T*)st->xkv.p + (int64_t)(2 * l + 1) * xkv_slab, st->da.p, B, H, Tn,
                                   st->skip_done ? st->done.as<int32_t>() : nullptr, var ? st->wc_dec.as<int32_t>() : nullptr, s, n_new);
        ++st->tally_xchunk;
      } else {
        ++st->tally_xattn[launch_cross_attn<T>(st->dq.p, (const T*)st->xkv.p + (int64_t)(2 * l) * xkv_slab, (const T*)st->xkv.p + (int64_t)(2 * l + 1) * xkv_slab,
                                               st->da.p, M, n_new, H, Tn, st->xa_part.as<float>(), st->xa_ticket.as<unsigned>(), st->xa_rows,
                                               kv_group > 1 ? win_done : (st->skip_done ? st->done.as<int32_t>() : nullptr), s, kv_group, st->batch_invariant,
                                               var ? st->wc_dec.as<int32_t>() : nullptr)];
      }
    }
    gemm(DT_XO, st->da.p, nullptr, w.wxo, w.bxo, st->dx.p, d, d, DEPI_BIAS_RESID, d);
    gemm(DT_FC1, st->dx.p, &w.ln2, w.w1, w.b1, st->df.p, 4 * d, d, DEPI_BIAS_GELU_T, 4 * d, &w.s1);
    gemm(DT_FC2, st->df.p, nullptr, w.w2, w.b2, st->dx.p, d, 4 * d, DEPI_BIAS_RESID, d);
  }
  if (!want_logits) return;
  launch_layernorm<T>(st->dx.as<float>(), c->dec_ln.g.as<float>(), c->dec_ln.b.as<float>(), st->dy.p, M, d, s, true);
  DevBuf none;
  gemm(DT_LOGITS, st->dy.p, nullptr, c->emb, none, st->logits.p, hp.n_vocab, d, DEPI_LOGITS, st->logits_ld);
}

// the context table onto the device in the layout of the state's chunk size; host[b]: [prev] + the tokens of slot b, or empty
void window_prompt_upload(ohw_state* st, const std::vector<std::vector<int32_t>>& host) {
  const ohw_ctx* c = st->ctx;
  const size_t Q = (size_t)st->wp_chunk, batch = host.size(), MB = (size_t)st->max_batch;
  const size_t NC = ((size_t)c->hp.n_text_ctx / 2 + Q - 1) / Q;
  std::vector<int32_t> feed(NC * batch * Q, c->tok.eot), pos(NC * MB), lens(MB, 0);
  if (feed.size() * 4 > st->wp_feed.bytes || pos.size() * 4 > st->wp_pos.bytes) throw Error(OHW_E_INVALID_ARG, "window_prompt: the table exceeds its buffers");
  for (size_t b = 0; b < batch; ++b) {
    lens[b] = (int32_t)host[b].size();
    for (size_t p = 0; p < host[b].size(); ++p) feed[((p / Q) * batch + b) * Q + p % Q] = host[b][p];
  }
  for (size_t j = 0; j < NC; ++j)
    for (size_t b = 0; b < MB; ++b) pos[j * MB + b] = (int32_t)(Q * j);
  HIP_CHECK(hipSetDevice(c->device));
  // in stream order behind the kernels that still read the previous table; the sources are vectors of this call, so wait
  HIP_CHECK(hipMemcpyAsync(st->wp_feed.p, feed.data(), feed.size() * 4, hipMemcpyHostToDevice, st->stream));
  HIP_CHECK(hipMemcpyAsync(st->wp_pos.p, pos.data(), pos.size() * 4, hipMemcpyHostToDevice, st->stream));
  HIP_CHECK(hipMemcpyAsync(st->wp_lens.p, lens.data(), lens.size() * 4, hipMemcpyHostToDevice, st->stream));
  HIP_CHECK(hipStreamSynchronize(st->stream));
  st->wp_len.assign(lens.begin(), lens.begin() + (long)batch);
}

// the text context of the table (ohw_state_set_window_prompt) through the decoder in chunks of Q = 8 or 16 positions
// (ohw_state_set_prefill_chunk): chunk j feeds positions Qj .. Qj + Q - 1 of every window at n_past = Qj ([eot] where a window's
// context has ended: those rows write cache positions at or past the window's length - at most len + Q - 1 <= n_text_ctx / 2 + 15,
// inside n_text_ctx - which the decode overwrites one by one before a query reads them), and names the windows it has nothing
// for - Qj >= len[b], or not active - in the done mask, so their cross K/V is not streamed.  No logits.  Leaves every layer's
// self K/V of positions 0 .. len[b] - 1 in cache row b; st->n_past and st->done are the caller's to set afterwards.
void run_prefill(ohw_state* st, int batch, const int32_t* active, const std::string& what) {
  if (st->wp_len.empty()) return;
  if ((int)st->wp_len.size() != batch)
    throw Error(OHW_E_INVALID_ARG, what + ": ohw_state_set_window_prompt named " + std::to_string(st->wp_len.size()) + " windows, the decode batch has " +
                                       std::to_string(batch));
  int max_len = 0;
  for (int b = 0; b < batch; ++b)
    if (!active || active[b]) max_len = std::max(max_len, st->wp_len[(size_t)b]);
  const int Q = st->wp_chunk;
  const int nc = (max_len + Q - 1) / Q;
  if (nc == 0) return;
  const size_t MB = (size_t)st->max_batch;
  hipStream_t s = st->stream;
  std::vector<int32_t> done((size_t)nc * MB, 1);
  for (int j = 0; j < nc; ++j)
    for (int b = 0; b < batch; ++b) done[(size_t)j * MB + b] = ((active && !active[b]) || Q * j >= st->wp_len[(size_t)b]) ? 1 : 0;
  HIP_CHECK(hipMemcpyAsync(st->wp_done.p, done.data(), done.size() * 4, hipMemcpyHostToDevice, s));
  SkipDone skip_done(st->skip_done);
  Dispatch::run(st->ctx->dtype, [&](auto* tag) {
    using T = std::remove_pointer_t<decltype(tag)>;
    for (int j = 0; j < nc; ++j) {
      HIP_CHECK(hipMemcpyAsync(st->n_past.p, st->wp_pos.as<int32_t>() + (size_t)j * MB, (size_t)batch * 4, hipMemcpyDeviceToDevice, s));
      HIP_CHECK(hipMemcpyAsync(st->done.p, st->wp_done.as<int32_t>() + (size_t)j * MB, (size_t)batch * 4, hipMemcpyDeviceToDevice, s));
      run_decoder_step<T>(st, batch, Q, st->wp_feed.as<int32_t>() + (size_t)j * batch * Q, 1, nullptr, nullptr, false, true);
    }
  });
  HIP_CHECK(hipStreamSynchronize(s));     // `done` is a stack-lifetime source
}
// the largest context of the table (0: none set)
int window_prompt_max(const ohw_state* st) {
  int m = 0;
  for (int32_t n : st->wp_len) m = std::max(m, (int)n);
  return m;
}

// after a stream synchronisation: did a workgroup of a persistent decoder step give up waiting (decode_persist.hip)?  Loud.
void persist_check(ohw_state* st) {
  if (!st->ps_words.p || st->persist_launches == 0) return;
  unsigned w = 0;
  HIP_CHECK(hipMemcpy(&w, st->ps_words.as<unsigned>() + 8, 4, hipMemcpyDeviceToHost));
  if (w != 0) {
    const unsigned zero = 0;
    (void)hipMemcpy(st->ps_words.as<unsigned>() + 8, &zero, 4, hipMemcpyHostToDevice);
    throw Error(OHW_E_TRANSCRIBE, "persistent decoder step: a workgroup gave up waiting in layer " + std::to_string((w - 1) / 10) + ", phase " +
                                      std::to_string((w - 1) % 10) + " (are all workgroups resident? OHW_DEC_PERSIST=0 selects the launch-per-kernel path)");
  }
}

void fill_sampler(const ohw_state* st, const ohw_sample_params* sp, int B, SamplerParams* p) {
  const ohw_ctx* c = st->ctx;
  std::memset(p, 0, sizeof *p);     // every byte, padding included: the graph caches compare these structs with memcmp
  p->logits = st->logits.as<float>(); p->ld = st->logits_ld;
  p->tokens = st->tokens.as<int32_t>(); p->n_cur = st->n_cur.as<int32_t>(); p->n_past = st->n_past.as<int32_t>();
  p->next_tok = st->next_tok.as<int32_t>(); p->done = st->done.as<int32_t>(); p->n_done = st->n_done.as<int32_t>();
  p->sum_logprob = st->sum_lp.as<float>();
  p->partials = st->samp_part.as<float>(); p->tickets = st->samp_ticket.as<unsigned>();
  p->bias = st->rules.bias_device();
  p->tok_lp = st->tok_lp.as<float>(); p->nosp_prob = st->nosp_prob.as<float>();
  p->batch = B; p->max_tokens = st->max_tokens; p->n_vocab = c->hp.n_vocab;
  p->eot = c->tok.eot; p->sot = c->tok.sot; p->translate = c->tok.translate; p->transcribe = c->tok.transcribe;
  p->solm = c->tok.solm; p->prev = c->tok.prev; p->nosp = c->tok.nosp; p->no_ts = c->tok.no_timestamps;
  p->ts_begin = c->tok.timestamp_begin; p->blank = c->tok.blank; p->n_langs = c->tok.n_langs;
  p->suppress_blank = sp->suppress_blank; p->no_timestamps = sp->no_timestamps; p->max_initial_ts = sp->max_initial_ts;
  p->n_max = sp->n_max; p->force_len = sp->force_len; p->n_text_ctx = c->hp.n_text_ctx;
}

int build_prompt(const ohw_ctx* c, const ohw_sample_params* sp, int32_t* out) {
  int n = 0;
  out[n++] = c->tok.sot;
  if (c->hp.n_vocab >= 51865) {
    out[n++] = c->tok.sot + 1 + sp->lang_id;
    out[n++] = sp->translate ? c->tok.translate : c->tok.transcribe;
  }
  if (sp->no_timestamps) out[n++] = c->tok.no_timestamps;
  return n;
}
// the same rows under a language table, written on the device: step_tok[b][0 .. n_prompt) with window b's own language token
void fill_prompt_rows(ohw_state* st, const ohw_sample_params* sp, int windows, int n_prompt) {
  const ohw_ctx* c = st->ctx;
  const int n = launch_prompt_fill(st->lang_tab.as<int32_t>(), st->step_tok.as<int32_t>(), windows, c->tok.sot, c->hp.n_vocab >= 51865 ? 1 : 0,
                                   sp->translate ? c->tok.translate : c->tok.transcribe, sp->no_timestamps ? c->tok.no_timestamps : -1, st->stream);
  if (n != n_prompt) throw Error(OHW_E_TRANSCRIBE, "prompt_fill: the device prompt has another length than build_prompt's");
}

// The start of a pass of a device decode loop (decode_loop, sample_pass_group, beam_search_run): the checks the three share,
// the prefill of the text contexts, the prompt rows in step_tok and the windows' start positions in n_past.  The caller has
// checked its pointers and its own arguments; what follows - its buffers, its first step - is its own.
struct PassOpts {
  const char* count = "n_windows";   // the name of the `windows` argument in the entry's messages
  int group = 1;                     // decoder rows per window, and that argument's name (null: the entry has no such argument)
  const char* group_name = nullptr;
  const int32_t* active = nullptr;   // a temperature pass: the windows it decodes (the prefill serves no others)
  int token_cap = INT32_MAX;         // a temperature pass: a row consumes at most this many draws
  bool timed = false;                // the pass is the one ohw_state_timings reports: its start is recorded
  int zero_rows = 0;                 // n_past is zeroed over this many rows first (beam search: the whole table)
};
struct PassSetup {
  int n_prompt = 0, n_max = 0;
  bool lang_tab = false;             // the rows' language tokens come from the state's table and sp->lang_id is ignored
  bool wp = false;                   // a text-context table is set (ohw_state_set_window_prompt)
  std::vector<int32_t> start;        // [windows] where window w's prompt starts: the length of its text context, or 0
  std::vector<int32_t> prompt_rows;  // the source of the prompt upload: it lives until the caller's next stream synchronisation
};
PassSetup begin_pass(ohw_state* st, const ohw_sample_params* sp, int windows, const char* what, const PassOpts& o) {
  const std::string w = what;
  if (windows < 1 || windows != st->enc_batch) throw Error(OHW_E_INVALID_ARG, w + ": " + o.count + " must equal the batch of the last ohw_encode");
  if (o.group_name && windows * o.group > st->max_batch)
    throw Error(OHW_E_INVALID_ARG, w + ": the state needs max_batch >= n_windows * " + o.group_name + " decoder rows");
  const ohw_ctx* c = st->ctx;
  check_decode_ctx(st, what);
  PassSetup ps;
  // under a language table the rows' language tokens come from device memory and sp->lang_id is ignored
  ps.lang_tab = !st->lang_kind.empty();
  if (ps.lang_tab) check_window_lang(st, windows, w);
  else if (sp->lang_id < 0 || sp->lang_id >= c->tok.n_langs) throw Error(OHW_E_INVALID_ARG, w + ": lang_id out of range");
  HIP_CHECK(hipSetDevice(c->device));
  hipStream_t s = st->stream;
  int32_t prompt[8];
  ohw_sample_params psp = *sp;
  if (ps.lang_tab) psp.lang_id = 0;
  ps.n_prompt = build_prompt(c, &psp, prompt);
  // under a text-context table window b starts at position wp_len[b]: the prefill puts the context there
  ps.wp = !st->wp_len.empty();
  const int n_max_raw = sp->force_len > 0 ? sp->force_len : sp->n_max;
  ps.n_max = std::min(std::min(std::min(n_max_raw, st->max_tokens), c->hp.n_text_ctx - ps.n_prompt - window_prompt_max(st)), o.token_cap);
  if (ps.n_max < 1) throw Error(OHW_E_INVALID_ARG, w + ": n_max < 1");
  if (o.timed) HIP_CHECK(hipEventRecord(st->ev[4], s));
  run_prefill(st, windows, o.active, w);     // checks the context table's batch
  ps.start.assign((size_t)windows, 0);
  if (ps.wp) ps.start = st->wp_len;
  if (ps.lang_tab) {
    fill_prompt_rows(st, &psp, windows, ps.n_prompt);
  } else {
    ps.prompt_rows.resize((size_t)windows * ps.n_prompt);
    for (int b = 0; b < windows; ++b) std::memcpy(&ps.prompt_rows[(size_t)b * ps.n_prompt], prompt, (size_t)ps.n_prompt * 4);
    HIP_CHECK(hipMemcpyAsync(st->step_tok.p, ps.prompt_rows.data(), ps.prompt_rows.size() * 4, hipMemcpyHostToDevice, s));
  }
  if (o.zero_rows > 0 || !ps.wp) HIP_CHECK(hipMemsetAsync(st->n_past.p, 0, (size_t)(o.zero_rows > 0 ? o.zero_rows : windows) * 4, s));
  if (ps.wp) HIP_CHECK(hipMemcpyAsync(st->n_past.p, st->wp_lens.p, (size_t)windows * 4, hipMemcpyDeviceToDevice, s));
  return ps;
}

// iterations 1 .. n_max - 1 of a device decode loop: launch(it) replays the captured graph or enqueues the kernels.  With
// `poll`, every eighth iteration reads n_done back and the loop leaves once it has reached `target`.  Returns the iterations run.
template <typename F>
int replay(ohw_state* st, int n_max, bool poll, int target, F&& launch) {
  hipStream_t s = st->stream;
  int32_t n_done_host = 0;
  int ran = 0;
  for (int it = 1; it < n_max; ++it) {
    launch(it);
    ++ran;
    if (poll && ((it & 7) == 7)) {
      HIP_CHECK(hipMemcpyAsync(&n_done_host, st->n_done.p, 4, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      if (n_done_host >= target) break;
    }
  }
  return ran;
}

// a beam step's pointers on a state's beam buffers; q: the side of the token-history, kv_slot and log-probability double buffers
// the step reads (it writes side q ^ 1).  nosp_prob stays null: the callers have their own rules for it
BeamParams beam_params(ohw_state* st, int K, int q, bool lp, int prefix_stride) {
  int32_t* tokbuf[2] = {st->tokens.as<int32_t>(), st->bm_tok2.as<int32_t>()};
  BeamParams bp{};
  bp.K = K; bp.prefix_stride = prefix_stride; bp.cand_lp = st->bm_cand_lp.as<float>(); bp.cand_tok = st->bm_cand_tok.as<int32_t>(); bp.beam_sum = st->bm_sum.as<float>();
  bp.kv_slot = st->bm_slot[q].as<int32_t>(); bp.kv_slot_next = st->bm_slot[q ^ 1].as<int32_t>(); bp.tokens_next = tokbuf[q ^ 1];
  bp.n_cur = st->bm_ncur.as<int32_t>(); bp.n_past_w = st->bm_npast.as<int32_t>(); bp.win_done = st->bm_done.as<int32_t>();
  bp.fin_cnt = st->bm_fin_cnt.as<int32_t>(); bp.fin_tok = st->bm_fin_tok.as<int32_t>(); bp.fin_len = st->bm_fin_len.as<int32_t>();
  bp.fin_sum = st->bm_fin_sum.as<float>();
  bp.part = st->bm_part.as<unsigned>(); bp.tickets = st->bm_ticket.as<unsigned>();
  if (lp) { bp.plog = st->bm_plog[q].as<float>(); bp.plog_next = st->bm_plog[q ^ 1].as<float>(); bp.fin_plog = st->bm_fin_plog.as<float>(); }
  return bp;
}

}  // namespace

// ================================================================================================
// C ABI
// ================================================================================================
extern "C" {

const char* ohw_last_error(void) { return g_last_error.c_str(); }
int ohw_abi_version(void) { return OHW_ABI_VERSION; }

int ohw_ctx_create(const char* model_path, int device, int dtype, ohw_ctx** out) {
  return guard([&] {
    if (!out) throw Error(OHW_E_INVALID_ARG, "out is null");
    *out = nullptr;
    *out = ctx_from_file(model_path, device, dtype);
  });
}

int ohw_ctx_create_synthetic(const ohw_hparams* hp, uint32_t seed, int device, int dtype, ohw_ctx** out) {
  return guard([&] {
    if (!out) throw Error(OHW_E_INVALID_ARG, "out is null");
    *out = nullptr;
    *out = ctx_synthetic(hp, seed, device, dtype);
  });
}

int ohw_ctx_info(const ohw_ctx* ctx, ohw_hparams* hp, ohw_special_tokens* tok) {
  return guard([&] {
    if (!ctx) throw Error(OHW_E_INVALID_ARG, "ctx is null");
    if (hp) *hp = ctx->hp;
    if (tok) *tok = ctx->tok;
  });
}

int ohw_ctx_dtype(const ohw_ctx* ctx) { return ctx ? ctx->dtype : OHW_E_INVALID_ARG; }

int ohw_token_text(const ohw_ctx* ctx, int32_t id, const char** text) {
  if (!ctx || id < 0 || (size_t)id >= ctx->vocab.size()) { if (text) *text = ""; return 0; }
  if (text) *text = ctx->vocab[(size_t)id].c_str();
  return (int)ctx->vocab[(size_t)id].size();
}

void ohw_ctx_free(ohw_ctx* ctx) {
  if (!ctx) return;
  ApiScope api;
  (void)hipSetDevice(ctx->device);
  delete ctx;
}

int ohw_state_create(ohw_ctx* ctx, int max_batch, ohw_state** out) {
  return guard([&] {
    if (!ctx || !out) throw Error(OHW_E_INVALID_ARG, "ctx/out is null");
    if (max_batch < 1 || max_batch > 256) throw Error(OHW_E_INVALID_ARG, "max_batch must be in 1..256");
    *out = nullptr;
    HIP_CHECK(hipSetDevice(ctx->device));
    std::unique_ptr<ohw_state> st(new ohw_state());
    st->ctx = ctx;
    st->max_batch = max_batch;
    st->rules.init(ctx->device, ctx->hp.n_vocab, ctx->tok.eot, max_batch, &st->stream);
    HIP_CHECK(hipStreamCreateWithFlags(&st->own_stream, hipStreamNonBlocking));
    st->stream = st->own_stream;
    state_alloc(st.get());
    HIP_CHECK(hipDeviceSynchronize());
    *out = st.release();
  });
}

void ohw_state_free(ohw_state* st) {
  if (!st) return;
  ApiScope api;
  (void)hipSetDevice(st->ctx->device);
  (void)hipDeviceSynchronize();
  for (auto& e : st->ev) if (e) (void)hipEventDestroy(e);
  for (auto& e : st->prof_ev) if (e) (void)hipEventDestroy(e);
  for (GraphCache* g : {&st->step_graphs, &st->group_graphs, &st->beam_graphs}) g->clear();
  if (st->own_stream) (void)hipStreamDestroy(st->own_stream);
  delete st;
}

int ohw_state_set_stream(ohw_state* st, void* hip_stream) {
  return guard([&] {
    if (!st) throw Error(OHW_E_INVALID_ARG, "state is null");
    st->stream = hip_stream ? (hipStream_t)hip_stream : st->own_stream;
    st->stream_cus = 0;
    if (hip_stream) {
      uint32_t mask[16] = {0};
      if (hipExtStreamGetCUMask(st->stream, 16, mask) == hipSuccess) {
        int n = 0, total = 0;
        for (uint32_t m : mask) n += __builtin_popcount(m);
        (void)hipDeviceGetAttribute(&total, hipDeviceAttributeMultiprocessorCount, st->ctx->device);
        if (n > 0 && n < total) st->stream_cus = n;
      } else {
        (void)hipGetLastError();
      }
    }

  });
}

int ohw_stream_create(int device, int first_cu, int n_cu, void** stream_out) {
  return guard([&] {
    if (!stream_out) throw Error(OHW_E_INVALID_ARG, "stream_out is null");
    *stream_out = nullptr;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) throw Error(OHW_E_NO_GPU, "stream: bad device index");
    HIP_CHECK(hipSetDevice(device));
    hipStream_t s = nullptr;
    if (n_cu <= 0) {
      HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    } else {
      hipDeviceProp_t prop;
      HIP_CHECK(hipGetDeviceProperties(&prop, device));
      const int total = prop.multiProcessorCount;
      if (first_cu < 0 || first_cu + n_cu > total) throw Error(OHW_E_INVALID_ARG, "stream: CU range exceeds the device's compute units");
      std::vector<uint32_t> mask((size_t)(total + 31) / 32, 0u);
      for (int b = first_cu; b < first_cu + n_cu; ++b) mask[(size_t)b / 32] |= 1u << (b % 32);
      HIP_CHECK(hipExtStreamCreateWithCUMask(&s, (uint32_t)mask.size(), mask.data()));
    }
    *stream_out = (void*)s;
  });
}
int ohw_stream_destroy(void* stream) {
  return guard([&] {
    if (stream) HIP_CHECK(hipStreamDestroy((hipStream_t)stream));
  });
}
int ohw_stream_wait(void* waiter, void* signal) {
  return guard([&] {
    if (!waiter || !signal) throw Error(OHW_E_INVALID_ARG, "stream is null");
    hipEvent_t e = nullptr;
    HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    hipError_t r = hipEventRecord(e, (hipStream_t)signal);
    if (r == hipSuccess) r = hipStreamWaitEvent((hipStream_t)waiter, e, 0);
    (void)hipEventDestroy(e);   // released once the recorded work has completed
    HIP_CHECK(r);
  });
}
int ohw_stream_sync(void* stream) {
  return guard([&] {
    if (!stream) throw Error(OHW_E_INVALID_ARG, "stream is null");
    HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  });
}

int ohw_state_max_batch(const ohw_state* st) { return st ? st->max_batch : 0; }
}  // extern "C"
namespace ohw {
// the state's logit bias as the host sampler needs it (null when none is set); library-internal
// dst reads src's recording (no copy: a view of its samples) and gets its maximum; same device; dst must not outlive src's
// recording (the engine shares among its own states for the length of one transcribe)
// lane states of the engine's LANES schedule: a graph capture waits until every other thread has left the library, i.e. until
// the other lanes' decodes are over - a lane only captures where the replay clearly pays (batches below `max_batch`)
void state_set_graph_max_batch(ohw_state* st, int max_batch) { if (st && max_batch >= 1) st->graph_max_batch = max_batch; }
void state_share_recording(ohw_state* dst, ohw_state* src) {
  if (!dst || !src || dst == src) return;
  if (src->rec_n < 1) throw Error(OHW_E_INVALID_ARG, "share_recording: the source state holds no recording");
  HIP_CHECK(hipSetDevice(src->ctx->device));
  HIP_CHECK(hipStreamSynchronize(src->stream));                 // the maximum is final
  dst->rec_pcm.view(src->rec_pcm.p, src->rec_pcm.bytes);
  dst->rec_n = src->rec_n;
  if (!dst->rec_max.p) dst->rec_max.alloc(4);
  if (dst->rec_off.bytes < (size_t)dst->max_batch * 8) dst->rec_off.alloc((size_t)dst->max_batch * 8);
  HIP_CHECK(hipMemcpy(dst->rec_max.p, src->rec_max.p, 4, hipMemcpyDeviceToDevice));
}
void state_drop_recording(ohw_state* st) {
  if (!st || st->rec_pcm.owned) return;
  st->rec_pcm.release();          // a view: nothing is freed
  st->rec_n = 0;
}
// a state's logit rules, for the engine: the host-sampled rung applies them and a transcribe syncs them across its states
LogitRules& state_rules(ohw_state* st) { return st->rules; }

// What the three rule test entries share (ohw_dbg_phrase_boost, ohw_dbg_repeat_rule, ohw_dbg_command_rule; include/ohw.h has
// their arguments).  Everything is range-checked first: the kernels index with these values.  Then, on the state's device and
// stream: upload() fills the entry's OWN LogitRules - a test entry never touches the state's -, logits, histories, n_cur and
// done are staged, launch() runs the kernel on them, and the logits come back whole
struct RuleRows {
  float* logits; int rows; int64_t ld; int n_vocab; const int32_t* histories; int max_tokens; const int32_t* n_cur; const int32_t* done;
  int n_entries, row_mul, group, eot;
};
template <typename U, typename L>
void dbg_rule_rows(ohw_state* st, const std::string& name, const RuleRows& a, int max_tokens_limit, int n_vocab_limit, U&& upload, L&& launch) {
  if (a.rows < 1 || a.rows > 4096 || a.n_vocab < 1 || a.n_vocab > n_vocab_limit || a.ld < a.n_vocab || a.max_tokens < 1 || a.max_tokens > max_tokens_limit ||
      a.eot < 0 || a.n_entries < 1 || a.n_entries > 4096 || a.row_mul < 1 || a.row_mul > 64 || a.group < 1 || a.group > 64)
    throw Error(OHW_E_INVALID_ARG, name + ": bad shape");
  if ((int64_t)(a.rows - 1) * a.row_mul / a.group >= a.n_entries) throw Error(OHW_E_INVALID_ARG, name + ": a launch row maps behind the last entry");
  for (int i = 0; a.n_cur && i < a.n_entries; ++i)
    if (a.n_cur[i] < 0 || a.n_cur[i] > a.max_tokens) throw Error(OHW_E_INVALID_ARG, name + ": n_cur out of range");
  HIP_CHECK(hipSetDevice(st->ctx->device));
  hipStream_t s = st->stream;
  HIP_CHECK(hipStreamSynchronize(s));
  upload();
  const size_t hist_rows = (size_t)a.n_entries * a.group, logit_bytes = (size_t)a.rows * a.ld * 4;
  DevBuf d_logits, d_hist, d_ncur, d_done;
  d_logits.alloc(logit_bytes); d_hist.alloc(hist_rows * a.max_tokens * 4); d_ncur.alloc((size_t)a.n_entries * 4); d_done.alloc((size_t)a.n_entries * 4);
  HIP_CHECK(hipMemcpyAsync(d_logits.p, a.logits, logit_bytes, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(d_hist.p, a.histories, hist_rows * a.max_tokens * 4, hipMemcpyHostToDevice, s));
  if (a.n_cur) HIP_CHECK(hipMemcpyAsync(d_ncur.p, a.n_cur, (size_t)a.n_entries * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(d_done.p, a.done, (size_t)a.n_entries * 4, hipMemcpyHostToDevice, s));
  launch(d_logits.as<float>(), d_hist.as<int32_t>(), a.n_cur ? d_ncur.as<int32_t>() : nullptr, d_done.as<int32_t>(), s);
  HIP_CHECK(hipMemcpyAsync(a.logits, d_logits.p, logit_bytes, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
}
}
extern "C" {
const ohw_ctx* ohw_state_ctx(const ohw_state* st) { return st ? st->ctx : nullptr; }

int ohw_mel(ohw_state* st, const float* pcm, int64_t pcm_stride, const int32_t* n_samples, int batch, int pcm_on_device,
            int mel_mode, float* mel_out) {
  return guard([&] {
    if (!st || !pcm || !n_samples) throw Error(OHW_E_INVALID_ARG, "null argument");
    if (batch < 1 || batch > st->max_batch) throw Error(OHW_E_INVALID_ARG, "batch exceeds the state's max_batch");
    if (mel_mode != OHW_MEL_REFLECT && mel_mode != OHW_MEL_ZERO_TAIL) throw Error(OHW_E_INVALID_ARG, "bad mel_mode");
    HIP_CHECK(hipSetDevice(st->ctx->device));
    hipStream_t s = st->stream;
    for (int b = 0; b < batch; ++b)
      if (n_samples[b] < 0 || n_samples[b] > CHUNK_SAMPLES || n_samples[b] > pcm_stride)
        throw Error(OHW_E_INVALID_ARG, "n_samples must be in 0..480000 and <= pcm_stride");
    HIP_CHECK(hipMemcpyAsync(st->n_samples.p, n_samples, (size_t)batch * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipEventRecord(st->ev[0], s));
    const float* pcm_dev = pcm;
    int64_t stride = pcm_stride;
    if (!pcm_on_device) {
      for (int b = 0; b < batch; ++b)
        if (n_samples[b] > 0)
          HIP_CHECK(hipMemcpyAsync(st->pcm.as<float>() + (int64_t)b * CHUNK_SAMPLES, pcm + (int64_t)b * pcm_stride,
                                   (size_t)n_samples[b] * 4, hipMemcpyHostToDevice, s));
      pcm_dev = st->pcm.as<float>();
      stride = CHUNK_SAMPLES;
    }
    Dispatch::run(st->ctx->dtype, [&](auto* tag) {
      using T = std::remove_pointer_t<decltype(tag)>;
      run_mel<T>(st, pcm_dev, stride, batch, mel_mode);
    });
    HIP_CHECK(hipEventRecord(st->ev[1], s));
    st->mel_batch = batch;
    st->enc_batch = batch;
    if (mel_out) {
      HIP_CHECK(hipMemcpyAsync(mel_out, st->logmel.p, (size_t)batch * st->ctx->hp.n_mels * CHUNK_FRAMES * 4, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
    }
  });
}

// ---- the spectral speech detector (vad.hip; include/ohw.h).  Scratch of its own: the state's recording, slots, mel and graphs
// are not touched ----
namespace {
VadParams vad_params(ohw_state* st, const float* pcm_dev, int64_t n, int64_t n_frames, int guard) {
  const size_t need = (size_t)(n_frames + guard) * 4;
  if (st->vad_e.bytes < need) st->vad_e.alloc(need);
  if (st->vad_p.bytes < need) st->vad_p.alloc(need);
  if (!st->vad_aux.p) st->vad_aux.alloc((VAD_BINS + 4) * 4);
  VadParams p{};
  p.pcm = pcm_dev; p.n = n; p.n_frames = n_frames;
  p.twiddle = st->ctx->twiddle.as<float>(); p.window = st->ctx->window.as<float>();
  p.energy = st->vad_e.as<float>(); p.prob = st->vad_p.as<float>();
  p.hist = st->vad_aux.as<int32_t>(); p.floor_db = st->vad_aux.as<float>() + VAD_BINS;
  return p;
}
// host samples go through the detector's own staging buffer; device samples are read where they are
const float* vad_stage_pcm(ohw_state* st, const float* pcm, int64_t n, int pcm_on_device, hipStream_t s) {
  if (pcm_on_device) return pcm;
  if (st->vad_pcm.bytes < (size_t)n * 4) st->vad_pcm.alloc((size_t)n * 4);
  HIP_CHECK(hipMemcpyAsync(st->vad_pcm.p, pcm, (size_t)n * 4, hipMemcpyHostToDevice, s));
  return st->vad_pcm.as<float>();
}
void vad_check_len(const float* pcm, int64_t n) {
  if (!pcm || n < 1) throw Error(OHW_E_INVALID_ARG, "vad: null or empty recording");
  if (n > (int64_t)7201 * 16000) throw Error(OHW_E_INVALID_ARG, "vad: more than two hours");
}
}  // namespace

void ohw_default_vad_detector(ohw_vad_detector* d) {
  if (!d) return;
  d->floor_quantile = 0.10f; d->margin_db = 9.0f; d->slope_db = 3.0f;
}

int ohw_state_vad_frames(ohw_state* st, const float* pcm, int64_t n, int pcm_on_device, const ohw_vad_detector* d, float* prob_out,
                         float* floor_db_out) {
  return guard([&] {
    if (!st || !prob_out) throw Error(OHW_E_INVALID_ARG, "vad_frames: null argument");
    vad_check_len(pcm, n);
    ohw_vad_detector det;
    if (d) det = *d; else ohw_default_vad_detector(&det);
    vad_detector_check(det);
    HIP_CHECK(hipSetDevice(st->ctx->device));
    hipStream_t s = st->stream;
    const int64_t n_frames = (n + HOP - 1) / HOP;
    const float* pcm_dev = vad_stage_pcm(st, pcm, n, pcm_on_device, s);
    VadParams p = vad_params(st, pcm_dev, n, n_frames, 0);
    p.target = vad_floor_target(det.floor_quantile, n_frames); p.margin_db = det.margin_db; p.slope_db = det.slope_db;
    launch_vad_band(p, s);
    launch_vad_floor_prob(p, s);
    HIP_CHECK(hipMemcpyAsync(prob_out, p.prob, (size_t)n_frames * 4, hipMemcpyDeviceToHost, s));
    if (floor_db_out) HIP_CHECK(hipMemcpyAsync(floor_db_out, p.floor_db, 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  });
}

// test entries: the detector's kernels alone, outputs sentinel-filled with guard space behind them (include/ohw.h)
int ohw_dbg_vad_energy(ohw_state* st, const float* pcm, int64_t n, int pcm_on_device, float* e_out, int guard_n) {
  return guard([&] {
    if (!st || !e_out) throw Error(OHW_E_INVALID_ARG, "dbg_vad_energy: null argument");
    if (guard_n < 0 || guard_n > 4096) throw Error(OHW_E_INVALID_ARG, "dbg_vad_energy: guard must be in 0..4096");
    vad_check_len(pcm, n);
    HIP_CHECK(hipSetDevice(st->ctx->device));
    hipStream_t s = st->stream;
    const int64_t n_frames = (n + HOP - 1) / HOP;
    const float* pcm_dev = vad_stage_pcm(st, pcm, n, pcm_on_device, s);
    const VadParams p = vad_params(st, pcm_dev, n, n_frames, guard_n);
    const std::vector<float> sent((size_t)(n_frames + guard_n), OHW_DBG_SENTINEL_F32);
    HIP_CHECK(hipMemcpyAsync(p.energy, sent.data(), sent.size() * 4, hipMemcpyHostToDevice, s));
    launch_vad_band(p, s);
    HIP_CHECK(hipMemcpyAsync(e_out, p.energy, sent.size() * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  });
}

int ohw_dbg_vad_floor(ohw_state* st, const float* e, int64_t n_frames, const ohw_vad_detector* d, float* prob_out, int guard_n, float* floor_db_out) {
  return guard([&] {
    if (!st || !e || !prob_out || !floor_db_out) throw Error(OHW_E_INVALID_ARG, "dbg_vad_floor: null argument");
    if (guard_n < 0 || guard_n > 4096) throw Error(OHW_E_INVALID_ARG, "dbg_vad_floor: guard must be in 0..4096");
    if (n_frames < 1 || n_frames > (int64_t)7201 * 100) throw Error(OHW_E_INVALID_ARG, "dbg_vad_floor: n_frames out of range");
    ohw_vad_detector det;
    if (d) det = *d; else ohw_default_vad_detector(&det);
    vad_detector_check(det);
    HIP_CHECK(hipSetDevice(st->ctx->device));
    hipStream_t s = st->stream;
    VadParams p = vad_params(st, nullptr, 0, n_frames, guard_n);
    p.target = vad_floor_target(det.floor_quantile, n_frames); p.margin_db = det.margin_db; p.slope_db = det.slope_db;
    const std::vector<float> sent((size_t)(n_frames + guard_n), OHW_DBG_SENTINEL_F32);
    HIP_CHECK(hipMemcpyAsync(p.energy, e, (size_t)n_frames * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(p.prob, sent.data(), sent.size() * 4, hipMemcpyHostToDevice, s));
    const float sent_f = OHW_DBG_SENTINEL_F32;
    HIP_CHECK(hipMemcpyAsync(p.floor_db, &sent_f, 4, hipMemcpyHostToDevice, s));
    launch_vad_floor_prob(p, s);
    HIP_CHECK(hipMemcpyAsync(prob_out, p.prob, sent.size() * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(floor_db_out, p.floor_db, 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  });
}

int ohw_recording_set(ohw_state* st, const float* pcm, int64_t n, int pcm_on_device, float* log_max_out) {
  return guard([&] {
    if (!st || !pcm || n < 1) throw Error(OHW_E_INVALID_ARG, "recording: null or empty");
    if (n > (int64_t)7200 * 16000) throw Error(OHW_E_INVALID_ARG, "recording: more than two hours");
    HIP_CHECK(hipSetDevice(st->ctx->device));
    hipStream_t s = st->stream;
    if (st->rec_pcm.bytes < (size_t)n * 4) st->rec_pcm.alloc((size_t)n * 4);
    HIP_CHECK(hipMemcpyAsync(st->rec_pcm.p, pcm, (size_t)n * 4, pcm_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    st->rec_n = n;
    // frames that touch a sample, in pseudo-windows of 3000; the frames of the 30 s zero tail are log10(1e-10) = -10
    const int64_t n_audio = (n + N_FFT / 2) / HOP + 1;
    const int chunks = (int)((n_audio + CHUNK_FRAMES - 1) / CHUNK_FRAMES);
    const size_t need = (size_t)std::max(chunks, st->max_batch) * 8;
    if (st->rec_off.bytes < need) st->rec_off.alloc(need);
    if (!st->rec_max.p) st->rec_max.alloc(4);
    std::vector<int64_t> offs((size_t)chunks);
    for (int i = 0; i < chunks; ++i) offs[(size_t)i] = (int64_t)i * CHUNK_SAMPLES;
    const float floor_v = -10.0f;
    int32_t floor_bits;
    std::memcpy(&floor_bits, &floor_v, 4);
    floor_bits ^= 0x7fffffff;                      // the kernels' ordered-int form of a negative float
    HIP_CHECK(hipMemcpyAsync(st->rec_max.p, &floor_bits, 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->rec_off.p, offs.data(), offs.size() * 8, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));            // offs and floor_bits are stack-lifetime sources
    const ohw_ctx* c = st->ctx;
    MelParams p{};
    p.pcm = st->rec_pcm.as<float>(); p.n_samples = st->n_samples.as<int32_t>();
    p.filters = c->mel_filters.as<float>(); p.twiddle = c->twiddle.as<float>(); p.window = c->window.as<float>();
    p.logmel = st->logmel.as<float>(); p.max_bits = st->rec_max.as<int32_t>(); p.mel_t = st->mel_t.p;
    p.n_mels = c->hp.n_mels; p.batch = chunks; p.mode = OHW_MEL_ZERO_TAIL;
    p.offsets = st->rec_off.as<int64_t>(); p.n_total = n; p.shared_max = 1; p.max_only = 1;
    Dispatch::run(c->dtype, [&](auto* tag) {
      using T = std::remove_pointer_t<decltype(tag)>;
      launch_mel<T>(p, s);
    });
    if (log_max_out) {
      int32_t bits = 0;
      HIP_CHECK(hipMemcpyAsync(&bits, st->rec_max.p, 4, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      if (bits < 0) bits ^= 0x7fffffff;
      std::memcpy(log_max_out, &bits, 4);
    }
  });
}

int ohw_mel_seek(ohw_state* st, const int32_t* seek_frames, int batch, float* mel_out) {
  return guard([&] {
    if (!st || !seek_frames) throw Error(OHW_E_INVALID_ARG, "null argument");
    if (st->rec_n < 1) throw Error(OHW_E_INVALID_ARG, "mel_seek: no recording (ohw_recording_set)");
    if (batch < 1 || batch > st->max_batch) throw Error(OHW_E_INVALID_ARG, "batch exceeds the state's max_batch");
    const int64_t n_len = (st->rec_n + CHUNK_SAMPLES) / HOP;
    std::vector<int64_t> offs((size_t)batch);
    for (int b = 0; b < batch; ++b) {
      if (seek_frames[b] < 0 || seek_frames[b] >= n_len) throw Error(OHW_E_INVALID_ARG, "mel_seek: seek outside the recording's frames");
      offs[(size_t)b] = (int64_t)seek_frames[b] * HOP;
    }
    HIP_CHECK(hipSetDevice(st->ctx->device));
    hipStream_t s = st->stream;
    HIP_CHECK(hipEventRecord(st->ev[0], s));
    HIP_CHECK(hipMemcpyAsync(st->rec_off.p, offs.data(), offs.size() * 8, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
    const ohw_ctx* c = st->ctx;
    MelParams p{};
    p.pcm = st->rec_pcm.as<float>(); p.n_samples = st->n_samples.as<int32_t>();
    p.filters = c->mel_filters.as<float>(); p.twiddle = c->twiddle.as<float>(); p.window = c->window.as<float>();
    p.logmel = st->logmel.as<float>(); p.max_bits = st->rec_max.as<int32_t>(); p.mel_t = st->mel_t.p;
    p.n_mels = c->hp.n_mels; p.batch = batch; p.mode = OHW_MEL_ZERO_TAIL;
    p.offsets = st->rec_off.as<int64_t>(); p.n_total = st->rec_n; p.shared_max = 1; p.max_only = 0;
    p.frame_limit = 2 * audio_ctx_of(st);
    p.win_ctx = mel_win_ctx(st, batch);
    st->mel_ctx = audio_ctx_of(st);
    st->mel_win = st->win_ctx;
    Dispatch::run(c->dtype, [&](auto* tag) {
      using T = std::remove_pointer_t<decltype(tag)>;
      launch_mel<T>(p, s);
    });
    HIP_CHECK(hipEventRecord(st->ev[1], s));
    st->mel_batch = batch;
    st->enc_batch = batch;
    if (mel_out) {
      HIP_CHECK(hipMemcpyAsync(mel_out, st->logmel.p, (size_t)batch * c->hp.n_mels * CHUNK_FRAMES * 4, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
    }
  });
}

// the slot calls' table buffer: four tables of `entries` rows each, one upload per call
static void slot_tab_reserve(ohw_state* st, int64_t entries) {
  if (st->slot_tab_entries >= entries) return;
  st->slot_tab.alloc((size_t)entries * 28);
  st->slot_tab_entries = entries;
}

int ohw_recording_set_slot(ohw_state* st, int slot, const float* pcm, int64_t n, int pcm_on_device, float* log_max_out) {
  return guard([&] {
    if (!st || !pcm || n < 1) throw Error(OHW_E_INVALID_ARG, "recording slot: null or empty");
    if (slot < 0 || slot >= st->max_batch)
      throw Error(OHW_E_INVALID_ARG, "recording slot: slot " + std::to_string(slot) + " of a state of " + std::to_string(st->max_batch));
    if (n > (int64_t)7200 * 16000) throw Error(OHW_E_INVALID_ARG, "recording slot: more than two hours");
    HIP_CHECK(hipSetDevice(st->ctx->device));
    hipStream_t s = st->stream;
    if (st->slot_pcm.empty()) {
      st->slot_pcm.resize((size_t)st->max_batch);
      st->slot_n.assign((size_t)st->max_batch, 0);
      st->slot_max.alloc((size_t)st->max_batch * 4);
    }
    st->slot_cap = std::max(st->slot_cap, n);
    DevBuf& buf = st->slot_pcm[(size_t)slot];
    st->slot_n[(size_t)slot] = 0;                    // empty until the new recording and its maximum are in place
    if (buf.bytes < (size_t)n * 4) {
      HIP_CHECK(hipStreamSynchronize(s));            // windows of the old recording may still be in flight
      buf.alloc((size_t)st->slot_cap * 4);
    }
    HIP_CHECK(hipMemcpyAsync(buf.p, pcm, (size_t)n * 4, pcm_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    // the maximum pass of ohw_recording_set, on this slot's samples and this slot's entry of the table
    const int64_t n_audio = (n + N_FFT / 2) / HOP + 1;
    const int chunks = (int)((n_audio + CHUNK_FRAMES - 1) / CHUNK_FRAMES);
    slot_tab_reserve(st, std::max(chunks, st->max_batch));
    std::vector<int64_t> offs((size_t)chunks);
    for (int i = 0; i < chunks; ++i) offs[(size_t)i] = (int64_t)i * CHUNK_SAMPLES;
    const float floor_v = -10.0f;
    int32_t floor_bits;
    std::memcpy(&floor_bits, &floor_v, 4);
    floor_bits ^= 0x7fffffff;
    int32_t* max_entry = st->slot_max.as<int32_t>() + slot;
    HIP_CHECK(hipMemcpyAsync(max_entry, &floor_bits, 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->slot_tab.p, offs.data(), offs.size() * 8, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));              // offs and floor_bits are stack-lifetime sources
    const ohw_ctx* c = st->ctx;
    MelParams p{};
    p.pcm = buf.as<float>(); p.n_samples = st->n_samples.as<int32_t>();
    p.filters = c->mel_filters.as<float>(); p.twiddle = c->twiddle.as<float>(); p.window = c->window.as<float>();
    p.logmel = st->logmel.as<float>(); p.max_bits = max_entry; p.mel_t = st->mel_t.p;
    p.n_mels = c->hp.n_mels; p.batch = chunks; p.mode = OHW_MEL_ZERO_TAIL;
    p.offsets = st->slot_tab.as<int64_t>(); p.n_total = n; p.shared_max = 1; p.max_only = 1;
    Dispatch::run(c->dtype, [&](auto* tag) {
      using T = std::remove_pointer_t<decltype(tag)>;
      launch_mel<T>(p, s);
    });
    st->slot_n[(size_t)slot] = n;
    if (log_max_out) {
      int32_t bits = 0;
      HIP_CHECK(hipMemcpyAsync(&bits, max_entry, 4, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      if (bits < 0) bits ^= 0x7fffffff;
      std::memcpy(log_max_out, &bits, 4);
    }
  });
}

int ohw_mel_seek_slots(ohw_state* st, const int32_t* slots, const int32_t* seek_frames, int batch, float* mel_out) {
  return guard([&] {
    if (!st || !slots || !seek_frames) throw Error(OHW_E_INVALID_ARG, "null argument");
    if (batch < 1 || batch > st->max_batch) throw Error(OHW_E_INVALID_ARG, "batch exceeds the state's max_batch");
    const int64_t E = st->slot_tab_entries;
    std::vector<char> tab((size_t)std::max<int64_t>(E, 1) * 28);
    int64_t* offs = (int64_t*)tab.data();
    const float** ptrs = (const float**)(tab.data() + E * 8);
    int64_t* lens = (int64_t*)(tab.data() + E * 16);
    int32_t* midx = (int32_t*)(tab.data() + E * 24);
    for (int b = 0; b < batch; ++b) {
      const int sl = slots[b];
      if (sl < 0 || sl >= st->max_batch)
        throw Error(OHW_E_INVALID_ARG, "mel_seek_slots: window " + std::to_string(b) + " names slot " + std::to_string(sl) + " of a state of " + std::to_string(st->max_batch));
      if (st->slot_n.empty() || st->slot_n[(size_t)sl] < 1)
        throw Error(OHW_E_INVALID_ARG, "mel_seek_slots: slot " + std::to_string(sl) + " holds no recording (ohw_recording_set_slot)");
      const int64_t n_len = (st->slot_n[(size_t)sl] + CHUNK_SAMPLES) / HOP;
      if (seek_frames[b] < 0 || seek_frames[b] >= n_len)
        throw Error(OHW_E_INVALID_ARG, "mel_seek_slots: window " + std::to_string(b) + " seeks outside its recording's frames");
      offs[b] = (int64_t)seek_frames[b] * HOP;
      ptrs[b] = st->slot_pcm[(size_t)sl].as<float>();
      lens[b] = st->slot_n[(size_t)sl];
      midx[b] = sl;
    }
    HIP_CHECK(hipSetDevice(st->ctx->device));
    hipStream_t s = st->stream;
    HIP_CHECK(hipEventRecord(st->ev[0], s));
    HIP_CHECK(hipMemcpyAsync(st->slot_tab.p, tab.data(), tab.size(), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
    const ohw_ctx* c = st->ctx;
    const char* dtab = st->slot_tab.as<char>();
    MelParams p{};
    p.pcm = nullptr; p.n_samples = st->n_samples.as<int32_t>();
    p.filters = c->mel_filters.as<float>(); p.twiddle = c->twiddle.as<float>(); p.window = c->window.as<float>();
    p.logmel = st->logmel.as<float>(); p.max_bits = st->slot_max.as<int32_t>(); p.mel_t = st->mel_t.p;
    p.n_mels = c->hp.n_mels; p.batch = batch; p.mode = OHW_MEL_ZERO_TAIL;
    p.offsets = (const int64_t*)dtab; p.n_total = 0; p.shared_max = 1; p.max_only = 0;
    p.win_pcm = (const float* const*)(dtab + E * 8); p.win_len = (const int64_t*)(dtab + E * 16); p.win_max = (const int32_t*)(dtab + E * 24);
    p.frame_limit = 2 * audio_ctx_of(st);
    p.win_ctx = mel_win_ctx(st, batch);
    st->mel_ctx = audio_ctx_of(st);
    st->mel_win = st->win_ctx;
    Dispatch::run(c->dtype, [&](auto* tag) {
      using T = std::remove_pointer_t<decltype(tag)>;
      launch_mel<T>(p, s);
    });
    HIP_CHECK(hipEventRecord(st->ev[1], s));
    st->mel_batch = batch;
    st->enc_batch = batch;
    if (mel_out) {
      HIP_CHECK(hipMemcpyAsync(mel_out, st->logmel.p, (size_t)batch * c->hp.n_mels * CHUNK_FRAMES * 4, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
    }
  });
}

int ohw_encode_slice(ohw_state* st, int batch, int first, int total) {
  return guard([&] {
    if (!st) throw Error(OHW_E_INVALID_ARG, "state is null");
    if (batch < 1 || batch != st->mel_batch) throw Error(OHW_E_INVALID_ARG, "encode: batch must equal the batch of the last ohw_mel");
    if (first < 0 || total < first + batch || total > st->max_batch) throw Error(OHW_E_INVALID_ARG, "encode: slice exceeds the state's max_batch");
    if (st->mel_ctx != audio_ctx_of(st)) throw Error(OHW_E_INVALID_ARG, "encode: the audio context changed since the last ohw_mel: run it again");
    if (first > 0 && st->enc_ctx != audio_ctx_of(st)) throw Error(OHW_E_INVALID_ARG, "encode: the slices of one decode batch must share one audio context");
    if (st->win_ctx != st->mel_win) throw Error(OHW_E_INVALID_ARG, "encode: the per-window contexts changed since the last ohw_mel: run it again");
    const bool var = !st->win_ctx.empty();
    if (first > 0 && st->enc_var != var)
      throw Error(OHW_E_INVALID_ARG, "encode: the slices of one decode batch run all with or all without per-window contexts");
    HIP_CHECK(hipSetDevice(st->ctx->device));
    window_lang_after_encode(st);
    HIP_CHECK(hipEventRecord(st->ev[2], st->stream));
    Dispatch::run(st->ctx->dtype, [&](auto* tag) {
      using T = std::remove_pointer_t<decltype(tag)>;
      run_encode<T>(st, batch, first, total);
    });
    HIP_CHECK(hipEventRecord(st->ev[3], st->stream));
    st->enc_batch = total;
    st->al_batch = 0;                  // the aligned windows are no longer resident: "align_*" fetches end here
    st->sc_batch = 0;                  //   and so does "score_logits"
    st->enc_ctx = audio_ctx_of(st);
    st->enc_set = st->win_ctx;
    st->enc_var = var;
    if (var) std::copy(st->win_ctx.begin(), st->win_ctx.end(), st->enc_win.begin() + first);
  });
}

int ohw_encode(ohw_state* st, int batch) { return ohw_encode_slice(st, batch, 0, batch); }

int ohw_decode_active(ohw_state* st, const int32_t* tokens, int n_new, const int32_t* n_past, int batch, const int32_t* active,
                      float* logits_out) {
  return guard([&] {
    if (!st || !tokens || !n_past) throw Error(OHW_E_INVALID_ARG, "null argument");
    if (batch < 1 || batch != st->enc_batch) throw Error(OHW_E_INVALID_ARG, "decode: batch must equal the batch of the last ohw_encode");
    if (n_new < 1 || n_new > 8) throw Error(OHW_E_INVALID_ARG, "decode: n_new must be in 1..8");
    check_decode_ctx(st, "decode");
    const ohw_hparams& hp = st->ctx->hp;
    for (int b = 0; b < batch; ++b) {
      if (n_past[b] < 0 || n_past[b] + n_new > hp.n_text_ctx) throw Error(OHW_E_INVALID_ARG, "decode: position exceeds n_text_ctx");
      for (int i = 0; i < n_new; ++i)
        if (tokens[b * n_new + i] < 0 || tokens[b * n_new + i] >= hp.n_vocab) throw Error(OHW_E_INVALID_ARG, "decode: token id out of range");
    }
    HIP_CHECK(hipSetDevice(st->ctx->device));
    hipStream_t s = st->stream;
    HIP_CHECK(hipMemcpyAsync(st->step_tok.p, tokens, (size_t)batch * n_new * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->n_past.p, n_past, (size_t)batch * 4, hipMemcpyHostToDevice, s));
    // inactive windows ride along (their GEMM rows are free) but their cross K/V is not streamed: the done flags the
    // greedy loop uses for finished windows
    std::vector<int32_t> skip;
    SkipDone skip_done(st->skip_done, active != nullptr);
    if (active) {
      skip.resize((size_t)batch);
      for (int b = 0; b < batch; ++b) skip[(size_t)b] = active[b] ? 0 : 1;
      HIP_CHECK(hipMemcpyAsync(st->done.p, skip.data(), skip.size() * 4, hipMemcpyHostToDevice, s));
    }
    Dispatch::run(st->ctx->dtype, [&](auto* tag) {
      using T = std::remove_pointer_t<decltype(tag)>;
      run_decoder_step<T>(st, batch, n_new);
    });
    if (logits_out) {
      if (!active) {
        HIP_CHECK(hipMemcpy2DAsync(logits_out, (size_t)hp.n_vocab * 4, st->logits.p, (size_t)st->logits_ld * 4, (size_t)hp.n_vocab * 4,
                                   (size_t)batch, hipMemcpyDeviceToHost, s));
      } else {
        for (int b = 0; b < batch; ++b)
          if (active[b])
            HIP_CHECK(hipMemcpyAsync(logits_out + (size_t)b * hp.n_vocab, st->logits.as<float>() + (size_t)b * st->logits_ld, (size_t)hp.n_vocab * 4,
                                     hipMemcpyDeviceToHost, s));
      }
    }
    HIP_CHECK(hipStreamSynchronize(s));   // also keeps `skip` alive until its copy has run
    persist_check(st);
  });
}

int ohw_decode(ohw_state* st, const int32_t* tokens, int n_new, const int32_t* n_past, int batch, float* logits_out) {
  return ohw_decode_active(st, tokens, n_new, n_past, batch, nullptr, logits_out);
}

void ohw_default_sample_params(const ohw_ctx* ctx, ohw_sample_params* p) {
  if (!p) return;
  p->lang_id = 0; p->translate = 0; p->no_timestamps = 0; p->suppress_blank = 1; p->max_initial_ts = 50;
  p->n_max = ctx ? ctx->hp.n_text_ctx / 2 - 4 : 220;
  p->force_len = 0;
}

// what a device-resident loop left in the state's sampler buffers, rows 0 .. batch - 1, as an ohw_greedy_result
static void decode_read_back(ohw_state* st, int batch, int max_tokens, const ohw_greedy_result* res) {
    const ohw_ctx* c = st->ctx;
    hipStream_t s = st->stream;
    int32_t* tokens_out = res->tokens;
    int32_t* n_tokens_out = res->n_tokens;
    float* sum_logprob_out = res->sum_logprob;
    std::vector<int32_t> toks((size_t)batch * st->max_tokens), ncur((size_t)batch);
    HIP_CHECK(hipMemcpyAsync(toks.data(), st->tokens.p, toks.size() * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(ncur.data(), st->n_cur.p, ncur.size() * 4, hipMemcpyDeviceToHost, s));
    if (sum_logprob_out) HIP_CHECK(hipMemcpyAsync(sum_logprob_out, st->sum_lp.p, (size_t)batch * 4, hipMemcpyDeviceToHost, s));
    std::vector<int32_t> last((size_t)batch);
    std::vector<float> lps;
    HIP_CHECK(hipMemcpyAsync(last.data(), st->next_tok.p, last.size() * 4, hipMemcpyDeviceToHost, s));
    if (res->no_speech_prob) HIP_CHECK(hipMemcpyAsync(res->no_speech_prob, st->nosp_prob.p, (size_t)batch * 4, hipMemcpyDeviceToHost, s));
    if (res->token_logprobs) {
      lps.resize((size_t)batch * (st->max_tokens + 1));
      HIP_CHECK(hipMemcpyAsync(lps.data(), st->tok_lp.p, lps.size() * 4, hipMemcpyDeviceToHost, s));
    }
    HIP_CHECK(hipStreamSynchronize(s));
    persist_check(st);
    for (int b = 0; b < batch; ++b) {
      const int n = std::min(ncur[(size_t)b], max_tokens);
      n_tokens_out[b] = n;
      std::memcpy(tokens_out + (size_t)b * max_tokens, &toks[(size_t)b * st->max_tokens], (size_t)n * 4);
      const bool eot = last[(size_t)b] == c->tok.eot && ncur[(size_t)b] <= max_tokens;
      if (res->ended_by_eot) res->ended_by_eot[b] = eot ? 1 : 0;
      if (res->token_logprobs) {
        float* dst = res->token_logprobs + (size_t)b * (max_tokens + 1);
        const int m = std::min(n + (eot ? 1 : 0), max_tokens + 1);
        std::memcpy(dst, &lps[(size_t)b * (st->max_tokens + 1)], (size_t)m * 4);
      }
    }
}

// the device-resident decode loop of ohw_greedy_ex (tp == nullptr: arg-max) and of ohw_sample_pass (tp: one temperature pass
// over the windows tp->active names, drawing with tp->uniforms).  Throws; the entries wrap it in guard().
struct TempPass {
  float temperature;
  const int32_t* active;     // [batch]
  const double* uniforms;    // [batch][max_tokens]
};
static void decode_loop(ohw_state* st, const ohw_sample_params* sp, int batch, int max_tokens, const ohw_greedy_result* res, const TempPass* tp) {
    const char* what = tp ? "sample_pass" : "greedy";
    if (!st || !sp || !res || !res->tokens || !res->n_tokens) throw Error(OHW_E_INVALID_ARG, "null argument");
    if (tp && (!tp->active || !tp->uniforms || !(tp->temperature > 0.0f) || max_tokens < 1))
      throw Error(OHW_E_INVALID_ARG, "sample_pass: needs temperature > 0, active, uniforms and max_tokens >= 1");
    PassOpts po;
    po.count = "batch";
    po.timed = !tp;                                        // ohw_state_timings reports the T = 0 loop
    if (tp) { po.active = tp->active; po.token_cap = max_tokens; }
    const PassSetup ps = begin_pass(st, sp, batch, what, po);
    const ohw_ctx* c = st->ctx;
    hipStream_t s = st->stream;
    const int n_prompt = ps.n_prompt, n_max = ps.n_max;
    HIP_CHECK(hipMemsetAsync(st->n_cur.p, 0, (size_t)batch * 4, s));
    // a temperature pass: windows with active[b] == 0 start finished (cross-attention and the sampler skip them)
    std::vector<int32_t> done0;
    int32_t n_done0[4] = {0, 0, 0, 0};
    if (tp) {
      done0.resize((size_t)batch);
      for (int b = 0; b < batch; ++b) { done0[(size_t)b] = tp->active[b] ? 0 : 1; n_done0[0] += done0[(size_t)b]; }
      HIP_CHECK(hipMemcpyAsync(st->done.p, done0.data(), done0.size() * 4, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemcpyAsync(st->n_done.p, n_done0, 16, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemcpyAsync(st->samp_temp.p, &tp->temperature, 4, hipMemcpyHostToDevice, s));
      const int nu = std::min(max_tokens, st->max_tokens);
      HIP_CHECK(hipMemcpy2DAsync(st->samp_u.p, (size_t)st->max_tokens * 8, tp->uniforms, (size_t)max_tokens * 8, (size_t)nu * 8, (size_t)batch,
                                 hipMemcpyHostToDevice, s));
    } else {
      HIP_CHECK(hipMemsetAsync(st->done.p, 0, (size_t)batch * 4, s));
      HIP_CHECK(hipMemsetAsync(st->n_done.p, 0, 16, s));
    }
    HIP_CHECK(hipMemsetAsync(st->sum_lp.p, 0, (size_t)batch * 4, s));
    HIP_CHECK(hipMemsetAsync(st->next_tok.p, 0, (size_t)batch * 4, s));
    HIP_CHECK(hipMemsetAsync(st->nosp_prob.p, 0, (size_t)batch * 4, s));
    SamplerParams spar;
    ohw_sample_params eff = *sp;
    eff.n_max = n_max;
    if (eff.force_len > 0) eff.force_len = n_max;
    fill_sampler(st, &eff, batch, &spar);
    int steps = 0;
    SkipDone skip_done(st->skip_done);
    Dispatch::run(c->dtype, [&](auto* tag) {
      using T = std::remove_pointer_t<decltype(tag)>;
      run_decoder_step<T>(st, batch, n_prompt);
      std::vector<int32_t> np((size_t)batch, n_prompt);
      for (int b = 0; b < batch; ++b) np[(size_t)b] += ps.start[(size_t)b];
      HIP_CHECK(hipMemcpyAsync(st->n_past.p, np.data(), np.size() * 4, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipStreamSynchronize(s));  // np, the prompt rows (and a temperature pass's done0, n_done0, T, draws) are stack-lifetime sources
      ++steps;
      auto sample = [&](hipStream_t q) {
        st->rules.apply(st->logits.as<float>(), spar.ld, spar, batch, 1, 1, spar.n_cur, spar.done, q);
        if (tp) launch_sampler_t(spar, st->samp_temp.as<float>(), st->samp_u.as<double>(), q);
        else launch_sampler(spar, q);
      };
      spar.advance = 0;
      sample(s);                 // first token of every window from the prompt's logits
      spar.advance = 1;          // every later sampler call follows a single-token step
      // One greedy iteration = {feed next_tok, decoder step, sampler}.  It is launch-bound (about 260
      // short kernels), so it is captured once into a hipGraph and replayed; positions, tokens and
      // the done flags live in device memory, so the same graph serves every iteration.
      auto iteration = [&](int, hipStream_t q) {
        run_decoder_step<T>(st, batch, 1, st->next_tok.as<int32_t>());   // the token the sampler just wrote
        sample(q);
      };
      // batch < graph_max_batch in this loop alone: the bound keeps a lane's wide greedy batch from capturing, which waits for the other lanes' decodes (state_set_graph_max_batch)
      const bool use_graph = st->graphs_enabled && st->prof_class == 0 && s != nullptr && batch < st->graph_max_batch;
      hipGraphExec_t step_exec = nullptr;
      if (use_graph) step_exec = st->step_graphs.get_or_capture(st, graph_key(st, batch, 0, tp != nullptr, spar), 1, iteration).exec[0];
      // a forced length runs every iteration: no polling
      steps += replay(st, n_max, sp->force_len <= 0, batch, [&](int it) {
        if (use_graph) HIP_CHECK(hipGraphLaunch(step_exec, s));
        else iteration(it, s);
      });
    });
    if (!tp) HIP_CHECK(hipEventRecord(st->ev[5], s));
    decode_read_back(st, batch, max_tokens, res);
    if (!tp) st->last.decode_steps = steps;     // ohw_state_timings reports the T = 0 loop
}

int ohw_greedy_ex(ohw_state* st, const ohw_sample_params* sp, int batch, int max_tokens, const ohw_greedy_result* res) {
  return guard([&] { decode_loop(st, sp, batch, max_tokens, res, nullptr); });
}

int ohw_sample_pass(ohw_state* st, const ohw_sample_params* sp, int batch, int max_tokens, float temperature, const int32_t* active,
                    const double* uniforms, const ohw_greedy_result* out) {
  return guard([&] {
    const TempPass tp{temperature, active, uniforms};
    decode_loop(st, sp, batch, max_tokens, out, &tp);
  });
}

// ohw_sample_pass_n: one temperature pass with N candidates per window (best-of sampling).  The prefill and the prompt run once
// per window, as in beam_search_run; the N rows of window w then share that past through a kv_slot table that is CONSTANT for
// the pass (candidates never reorder) and the window's cross K/V (run_decoder_step with kv_group = N).  Nothing of the layout
// outlives the call: every decode entry sets n_past, the done flags, the histories and its own slot table (or none) itself
static void sample_pass_group(ohw_state* st, const ohw_sample_params* sp, int W, int N, int max_tokens, const TempPass& tp, const ohw_greedy_result* res) {
    if (!st || !sp || !res || !res->tokens || !res->n_tokens) throw Error(OHW_E_INVALID_ARG, "null argument");
    const int R = W * N;
    if (N < 2 || N > 5) throw Error(OHW_E_INVALID_ARG, "sample_pass_n: best_of must be in 1..5");
    if (!tp.active || !tp.uniforms || !(tp.temperature > 0.0f) || max_tokens < 1)
      throw Error(OHW_E_INVALID_ARG, "sample_pass_n: needs temperature > 0, active, uniforms and max_tokens >= 1");
    if (sp->force_len > 0) throw Error(OHW_E_INVALID_ARG, "sample_pass_n: force_len is a single-candidate knob");
    const ohw_ctx* c = st->ctx;
    HIP_CHECK(hipSetDevice(c->device));
    const int C = c->hp.n_text_ctx, MB = st->max_batch;
    if (!st->sn_slot.p) { st->sn_slot.alloc((size_t)MB * C * 4, true); st->sn_win.alloc((size_t)MB * 4 * 4, true); }
    PassOpts po;                                      // the N rows of a window share its prompt; the prompt pass skips inactive windows
    po.group = N; po.group_name = "best_of";
    po.active = tp.active; po.token_cap = max_tokens;
    const PassSetup ps = begin_pass(st, sp, W, "sample_pass_n", po);
    hipStream_t s = st->stream;
    const int n_prompt = ps.n_prompt, n_max = ps.n_max;
    int32_t* d_shared = st->sn_win.as<int32_t>();
    int32_t* d_active = d_shared + MB;
    int32_t* d_wdone = d_shared + 2 * MB;
    unsigned* d_wcnt = (unsigned*)(d_shared + 3 * MB);
    std::vector<int32_t> shared((size_t)W), act((size_t)W), skip((size_t)W);
    int32_t n_done0[4] = {0, 0, 0, 0};
    for (int w = 0; w < W; ++w) {
      shared[(size_t)w] = ps.start[(size_t)w] + n_prompt;
      act[(size_t)w] = tp.active[w] ? 1 : 0;
      skip[(size_t)w] = act[(size_t)w] ? 0 : 1;
      n_done0[0] += skip[(size_t)w] * N;             // n_done counts rows
    }
    HIP_CHECK(hipMemcpyAsync(st->done.p, skip.data(), (size_t)W * 4, hipMemcpyHostToDevice, s));     // the prompt pass skips inactive windows
    HIP_CHECK(hipMemcpyAsync(st->n_done.p, n_done0, 16, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_shared, shared.data(), (size_t)W * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_active, act.data(), (size_t)W * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->samp_temp.p, &tp.temperature, 4, hipMemcpyHostToDevice, s));
    const int nu = std::min(max_tokens, st->max_tokens);
    HIP_CHECK(hipMemcpy2DAsync(st->samp_u.p, (size_t)st->max_tokens * 8, tp.uniforms, (size_t)max_tokens * 8, (size_t)nu * 8, (size_t)R, hipMemcpyHostToDevice, s));
    for (DevBuf* b : {&st->n_cur, &st->sum_lp, &st->next_tok, &st->nosp_prob}) HIP_CHECK(hipMemsetAsync(b->p, 0, (size_t)R * 4, s));
    SamplerParams spar;
    ohw_sample_params eff = *sp;
    eff.n_max = n_max;
    fill_sampler(st, &eff, R, &spar);
    SampGroup grp{N, d_wdone, d_wcnt};
    // under a context table the windows' pasts differ in length: window w's goes to row w * N, which only its own candidates
    // write (beam_search_run gives the reason)
    const int stride = (ps.wp && W > 1) ? N : 1;
    SampGroupInit gi{};
    gi.rows = R; gi.group = N; gi.n_ctx = C; gi.prefix_stride = stride; gi.shared = d_shared; gi.active = d_active;
    gi.kv_slot = st->sn_slot.as<int32_t>(); gi.n_past = st->n_past.as<int32_t>(); gi.done = st->done.as<int32_t>(); gi.win_done = d_wdone; gi.win_cnt = d_wcnt;
    const int32_t* slots = st->sn_slot.as<int32_t>();
    Dispatch::run(c->dtype, [&](auto* tag) {
      using T = std::remove_pointer_t<decltype(tag)>;
      {
        SkipDone skip_done(st->skip_done);
        run_decoder_step<T>(st, W, n_prompt);                     // the prompt once per window; its K/V stays in cache rows 0 .. W-1
      }
      if (stride > 1)
        for (int w = W - 1; w >= 1; --w)                          // from the last window down: row w * N < W is a later window's source
          launch_kv_prefix_move<T>(st->self_kv.p, 2 * c->hp.n_text_layer, MB, c->hp.n_text_head, C, w, w * N, shared[(size_t)w], s);
      launch_sample_group_init(gi, s);                            // slot table, n_past and done per row, the windows' flags
      st->sn_rows = R;
      HIP_CHECK(hipStreamSynchronize(s));                         // the vectors above and the prompt rows are stack-lifetime sources
      spar.advance = 0;
      // the candidates share the window's prompt row and their histories are empty: once per window
      st->rules.apply(st->logits.as<float>(), spar.ld, spar, W, 1, 1, nullptr, d_wdone, s);
      launch_sampler_group(spar, grp, st->samp_temp.as<float>(), st->samp_u.as<double>(), s);   // first token of every row from its window's prompt logits
      spar.advance = 1;
      auto iteration = [&](int, hipStream_t q) {
        run_decoder_step<T>(st, R, 1, st->next_tok.as<int32_t>(), N, slots, d_wdone);
        st->rules.apply(st->logits.as<float>(), spar.ld, spar, R, 1, 1, spar.n_cur, spar.done, q, N);     // a window's N candidates are neighbours
        launch_sampler_group(spar, grp, st->samp_temp.as<float>(), st->samp_u.as<double>(), q);
      };
      const bool use_graph = st->graphs_enabled && st->prof_class == 0 && s != nullptr;
      hipGraphExec_t step_exec = nullptr;
      if (use_graph) step_exec = st->group_graphs.get_or_capture(st, graph_key(st, W, N, true, spar), 1, iteration).exec[0];
      replay(st, n_max, true, R, [&](int it) {
        if (use_graph) HIP_CHECK(hipGraphLaunch(step_exec, s));
        else iteration(it, s);
      });
    });
    decode_read_back(st, R, max_tokens, res);
}

int ohw_sample_pass_n(ohw_state* st, const ohw_sample_params* sp, int n_windows, int best_of, int max_tokens, float temperature,
                      const int32_t* active, const double* uniforms, const ohw_greedy_result* out) {
  if (best_of == 1) return ohw_sample_pass(st, sp, n_windows, max_tokens, temperature, active, uniforms, out);
  return guard([&] {
    const TempPass tp{temperature, active, uniforms};
    sample_pass_group(st, sp, n_windows, best_of, max_tokens, tp, out);
  });
}

int ohw_greedy(ohw_state* st, const ohw_sample_params* sp, int batch, int32_t* tokens_out, int32_t* n_tokens_out, int max_tokens,
               float* sum_logprob_out) {
  ohw_greedy_result r{};
  r.tokens = tokens_out; r.n_tokens = n_tokens_out; r.sum_logprob = sum_logprob_out;
  return ohw_greedy_ex(st, sp, batch, max_tokens, &r);
}

// the beam search's buffers of a state, allocated at first use (ohw_beam_search, ohw_dbg_beam_step)
static void alloc_beam_buffers(ohw_state* st) {
  if (st->bm_sum.p) return;
  const size_t MT = (size_t)st->max_tokens, C = (size_t)st->ctx->hp.n_text_ctx, MB = (size_t)st->max_batch;
  st->bm_cand_lp.alloc(MB * 6 * 4); st->bm_cand_tok.alloc(MB * 6 * 4); st->bm_sum.alloc(MB * 4, true);
  st->bm_slot[0].alloc(MB * C * 4, true); st->bm_slot[1].alloc(MB * C * 4, true); st->bm_tok2.alloc(MB * MT * 4, true);
  st->bm_ncur.alloc(MB * 4, true); st->bm_npast.alloc(MB * 4, true); st->bm_done.alloc(MB * 4, true);
  st->bm_fin_cnt.alloc(MB * 4, true); st->bm_fin_tok.alloc(MB * MT * 4, true); st->bm_fin_len.alloc(MB * 4, true);
  st->bm_fin_sum.alloc(MB * 4, true);
  st->bm_part.alloc(MB * BEAM_SPLIT * BEAM_PART_WORDS * 4, true); st->bm_ticket.alloc(MB * 4, true);
  st->bm_plog[0].alloc(MB * (MT + 1) * 4, true); st->bm_plog[1].alloc(MB * (MT + 1) * 4, true); st->bm_fin_plog.alloc(MB * (MT + 1) * 4, true);
  st->bm_out_tok.alloc(MB * MT * 4, true); st->bm_out_lp.alloc(MB * (MT + 1) * 4, true);
  for (DevBuf* b : {&st->bm_out_n, &st->bm_out_sum, &st->bm_out_eot, &st->bm_out_nfin, &st->bm_nosp}) b->alloc(MB * 4, true);
}

// the device-side ranking on a state's beam buffers; last_q: the half of the double buffers that holds the live beams
static BeamFinishParams finish_params(ohw_state* st, int K, int max_tokens, int last_q) {
  BeamFinishParams f{};
  f.K = K; f.stride = st->max_tokens; f.max_tokens = std::min(max_tokens, st->max_tokens);
  f.fin_cnt = st->bm_fin_cnt.as<int32_t>(); f.fin_len = st->bm_fin_len.as<int32_t>(); f.fin_tok = st->bm_fin_tok.as<int32_t>();
  f.n_cur = st->bm_ncur.as<int32_t>(); f.tokens = last_q ? st->bm_tok2.as<int32_t>() : st->tokens.as<int32_t>();
  f.fin_sum = st->bm_fin_sum.as<float>(); f.fin_plog = st->bm_fin_plog.as<float>(); f.beam_sum = st->bm_sum.as<float>();
  f.plog = st->bm_plog[last_q].as<float>();
  f.out_tok = st->bm_out_tok.as<int32_t>(); f.out_n = st->bm_out_n.as<int32_t>(); f.out_eot = st->bm_out_eot.as<int32_t>();
  f.out_nfin = st->bm_out_nfin.as<int32_t>(); f.out_lp = st->bm_out_lp.as<float>(); f.out_sum = st->bm_out_sum.as<float>();
  return f;
}

// ohw_beam_search (ex null: no log-probability history, the final ranking on the host) and ohw_beam_search_ex (ex set: res is
// unused) are ONE search; what differs is which pointers the step kernels get and where the winner is picked
static void beam_search_run(ohw_state* st, const ohw_sample_params* sp, int n_windows, int beam_size, int max_tokens, const ohw_beam_result* res,
                            const ohw_beam_result_ex* ex) {
  {
    if (!st || !sp) throw Error(OHW_E_INVALID_ARG, "null argument");
    if (ex ? (!ex->tokens || !ex->n_tokens) : (!res || !res->tokens || !res->n_tokens)) throw Error(OHW_E_INVALID_ARG, "null argument");
    if (max_tokens < 0) throw Error(OHW_E_INVALID_ARG, "beam search: max_tokens < 0");
    const bool lp = ex != nullptr;
    const int W = n_windows, K = beam_size, R = W * K;
    if (K < 2 || K > 5) throw Error(OHW_E_INVALID_ARG, "beam search: beam_size must be in 2..5");
    if (sp->force_len > 0) throw Error(OHW_E_INVALID_ARG, "beam search: force_len is a greedy-only knob");
    const ohw_ctx* c = st->ctx;
    HIP_CHECK(hipSetDevice(c->device));
    const int MT = st->max_tokens, C = c->hp.n_text_ctx, MB = st->max_batch;
    alloc_beam_buffers(st);
    PassOpts po;                                      // all K rows of a window share its prompt and its language table entry
    po.group = K; po.group_name = "beam_size";
    po.timed = true;
    po.zero_rows = MB;
    const PassSetup ps = begin_pass(st, sp, W, "beam search", po);     // n_max is not clamped to max_tokens: the ranking truncates
    hipStream_t s = st->stream;
    const int n_prompt = ps.n_prompt, n_max = ps.n_max;
    // under a text-context table window w's prompt starts at position wp_len[w]; the context's K/V lives in slot w like the prompt's
    const bool wp = ps.wp;
    std::vector<int32_t> np0((size_t)W);
    for (int w = 0; w < W; ++w) np0[(size_t)w] = ps.start[(size_t)w] + n_prompt - 1;
    HIP_CHECK(hipMemsetAsync(st->n_done.p, 0, 16, s));
    for (DevBuf* b : {&st->bm_sum, &st->bm_ncur, &st->bm_done, &st->bm_fin_cnt, &st->bm_fin_len}) HIP_CHECK(hipMemsetAsync(b->p, 0, (size_t)MB * 4, s));
    HIP_CHECK(hipMemcpyAsync(st->bm_npast.p, np0.data(), np0.size() * 4, hipMemcpyHostToDevice, s));
    ohw_sample_params eff = *sp;
    eff.n_max = n_max;
    SamplerParams base;
    fill_sampler(st, &eff, R, &base);     // zeroes every byte first; advance stays 0: the beam step advances n_past itself
    int32_t* tokbuf[2] = {st->tokens.as<int32_t>(), st->bm_tok2.as<int32_t>()};
    auto params = [&](int q, SamplerParams* p, BeamParams* bp) {
      std::memcpy(p, &base, sizeof base);
      p->tokens = tokbuf[q];
      *bp = beam_params(st, K, q, lp, (wp && W > 1) ? K : 1);
      if (lp) bp->nosp_prob = st->bm_nosp.as<float>();      // read by the first step alone
    };
    int steps = 0, last_q = 1;
    Dispatch::run(c->dtype, [&](auto* tag) {
      using T = std::remove_pointer_t<decltype(tag)>;
      run_decoder_step<T>(st, W, n_prompt);                       // the prompt once per window; its K/V stays in cache rows 0 .. W-1
      // under a context table the windows' pasts differ in length, and cache row w (1 <= w < W) is also the own row of beam w % K of
      // window w / K, which writes from ITS past's end upward - into window w's context where that is longer.  So window w's past
      // moves to row w * K, which only w's beams write.  From the last window down: row w * K < W is a later window's source
      if (wp && W > 1)
        for (int w = W - 1; w >= 1; --w)
          launch_kv_prefix_move<T>(st->self_kv.p, 2 * c->hp.n_text_layer, st->max_batch, c->hp.n_text_head, C, w, w * K, np0[(size_t)w] + 1, s);
      HIP_CHECK(hipStreamSynchronize(s));                         // the prompt rows / np0 are stack-lifetime sources
      ++steps;
      SamplerParams p0; BeamParams b0;
      params(0, &p0, &b0);
      st->rules.apply(st->logits.as<float>(), p0.ld, p0, W, K, K, b0.n_cur, b0.win_done, s);
      launch_beam_step(p0, b0, W, 1, s);                          // first candidates from the prompt's logits; writes side 1
      // one beam iteration = {decoder step of the W * K rows, top-k per row, update per window}; the token-history and
      // kv_slot double buffers alternate, so TWO graphs are captured (odd and even steps) and replayed in turn
      const bool use_graph = st->graphs_enabled && st->prof_class == 0 && s != nullptr;
      hipGraphExec_t exec[2] = {nullptr, nullptr};
      if (use_graph) {
        const GraphEntry& g = st->beam_graphs.get_or_capture(st, graph_key(st, W, K, lp, base), 2, [&](int q, hipStream_t cap) {
          SamplerParams pq; BeamParams bq;
          params(q, &pq, &bq);
          run_decoder_step<T>(st, R, 1, st->next_tok.as<int32_t>(), K, bq.kv_slot, bq.win_done);
          BMARK("decoder step captured", q);
          st->rules.apply(st->logits.as<float>(), pq.ld, pq, R, 1, K, bq.n_cur, bq.win_done, cap);   // each beam's history in this step's half of the buffer
          launch_beam_step(pq, bq, W, 0, cap);
          BMARK("beam step captured", q);
        });
        exec[0] = g.exec[0]; exec[1] = g.exec[1];
      }
      const int ran = replay(st, n_max, true, W, [&](int it) {
        const int q = it & 1;
        if (use_graph) {
          BMARK("graph launch", it);
          HIP_CHECK(hipGraphLaunch(exec[q], s));
          BMARK("graph launched", it);
        } else {
          SamplerParams pq; BeamParams bq;
          params(q, &pq, &bq);
          run_decoder_step<T>(st, R, 1, st->next_tok.as<int32_t>(), K, bq.kv_slot, bq.win_done);
          st->rules.apply(st->logits.as<float>(), pq.ld, pq, R, 1, K, bq.n_cur, bq.win_done, s);
          launch_beam_step(pq, bq, W, 0, s);
        }
      });
      steps += ran;
      last_q = (ran & 1) ^ 1;                                     // the side the last iteration wrote (no iteration: the first step's side 1)
    });
    if (lp) {
      // the ranking on the device (beam_finish_kernel restates the host loop below); W rows come back
      launch_beam_finish(finish_params(st, K, max_tokens, last_q), W, s);
      HIP_CHECK(hipEventRecord(st->ev[5], s));
      const int n_copy = std::min(max_tokens, MT);
      if (n_copy > 0) HIP_CHECK(hipMemcpy2DAsync(ex->tokens, (size_t)max_tokens * 4, st->bm_out_tok.p, (size_t)MT * 4, (size_t)n_copy * 4, (size_t)W, hipMemcpyDeviceToHost, s));
      if (ex->token_logprobs)
        HIP_CHECK(hipMemcpy2DAsync(ex->token_logprobs, (size_t)(max_tokens + 1) * 4, st->bm_out_lp.p, (size_t)(MT + 1) * 4, (size_t)(n_copy + 1) * 4, (size_t)W, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipMemcpyAsync(ex->n_tokens, st->bm_out_n.p, (size_t)W * 4, hipMemcpyDeviceToHost, s));
      if (ex->sum_logprob) HIP_CHECK(hipMemcpyAsync(ex->sum_logprob, st->bm_out_sum.p, (size_t)W * 4, hipMemcpyDeviceToHost, s));
      if (ex->n_finished) HIP_CHECK(hipMemcpyAsync(ex->n_finished, st->bm_out_nfin.p, (size_t)W * 4, hipMemcpyDeviceToHost, s));
      if (ex->ended_by_eot) HIP_CHECK(hipMemcpyAsync(ex->ended_by_eot, st->bm_out_eot.p, (size_t)W * 4, hipMemcpyDeviceToHost, s));
      if (ex->no_speech_prob) HIP_CHECK(hipMemcpyAsync(ex->no_speech_prob, st->bm_nosp.p, (size_t)W * 4, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      persist_check(st);
      st->last.decode_steps = steps;
      return;
    }
    HIP_CHECK(hipEventRecord(st->ev[5], s));
    // read the finished pools and the live beams back; rank on the host: cumulative log-probability / length
    std::vector<int32_t> fin_cnt((size_t)W), fin_len((size_t)R), fin_tok((size_t)R * MT), live_tok((size_t)R * MT), ncur((size_t)W);
    std::vector<float> fin_sum((size_t)R), live_sum((size_t)R);
    HIP_CHECK(hipMemcpyAsync(fin_cnt.data(), st->bm_fin_cnt.p, (size_t)W * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(fin_len.data(), st->bm_fin_len.p, (size_t)R * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(fin_sum.data(), st->bm_fin_sum.p, (size_t)R * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(fin_tok.data(), st->bm_fin_tok.p, (size_t)R * MT * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(live_tok.data(), tokbuf[last_q], (size_t)R * MT * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(live_sum.data(), st->bm_sum.p, (size_t)R * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(ncur.data(), st->bm_ncur.p, (size_t)W * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    persist_check(st);
    for (int w = 0; w < W; ++w) {
      struct Cand { const int32_t* t; int n; float sum; };
      std::vector<Cand> cands;
      for (int f = 0; f < fin_cnt[(size_t)w]; ++f) cands.push_back({&fin_tok[(size_t)(w * K + f) * MT], fin_len[(size_t)(w * K + f)], fin_sum[(size_t)(w * K + f)]});
      if ((int)cands.size() < K) {
        // not enough finished sequences: the live beams join, most likely first (the published decoder's finalize())
        std::vector<int> order((size_t)K);
        for (int j = 0; j < K; ++j) order[(size_t)j] = j;
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return live_sum[(size_t)(w * K + a)] > live_sum[(size_t)(w * K + b)]; });
        for (int j : order) {
          if ((int)cands.size() >= K) break;
          if (!(live_sum[(size_t)(w * K + j)] > -INFINITY)) continue;
          cands.push_back({&live_tok[(size_t)(w * K + j) * MT], ncur[(size_t)w], live_sum[(size_t)(w * K + j)]});
        }
      }
      int best = -1;
      float best_score = -INFINITY;
      for (size_t i = 0; i < cands.size(); ++i) {
        const float score = cands[i].sum / (float)std::max(1, cands[i].n);
        if (best < 0 || score > best_score) { best = (int)i; best_score = score; }
      }
      const int n = best >= 0 ? std::min(cands[(size_t)best].n, max_tokens) : 0;
      res->n_tokens[w] = n;
      if (n) std::memcpy(res->tokens + (size_t)w * max_tokens, cands[(size_t)best].t, (size_t)n * 4);
      if (res->sum_logprob) res->sum_logprob[w] = best >= 0 ? cands[(size_t)best].sum : 0.f;
      if (res->n_finished) res->n_finished[w] = fin_cnt[(size_t)w];
    }
    st->last.decode_steps = steps;
  }
}

int ohw_beam_search(ohw_state* st, const ohw_sample_params* sp, int n_windows, int beam_size, int max_tokens, const ohw_beam_result* res) {
  return guard([&] { beam_search_run(st, sp, n_windows, beam_size, max_tokens, res, nullptr); });
}
int ohw_beam_search_ex(ohw_state* st, const ohw_sample_params* sp, int n_windows, int beam_size, int max_tokens, const ohw_beam_result_ex* out) {
  return guard([&] {
    if (!out) throw Error(OHW_E_INVALID_ARG, "null argument");
    beam_search_run(st, sp, n_windows, beam_size, max_tokens, nullptr, out);
  });
}

int ohw_dbg_counter(const ohw_state* st, const char* name) {
  if (!st || !name) return OHW_E_INVALID_ARG;
  const std::string n = name;
  if (n == "beam_captures") return st->beam_graphs.captures;
  if (n == "beam_graphs") return (int)st->beam_graphs.entries.size();
  if (n == "step_captures") return st->step_graphs.captures + st->group_graphs.captures;     // a group capture counts here too
  if (n == "step_graphs") return (int)st->step_graphs.entries.size();
  if (n == "group_graphs") return (int)st->group_graphs.entries.size();
  if (n == "persist_launches") return st->persist_launches;
  if (n == "xattn.chunk") return (int)std::min<int64_t>(st->tally_xchunk, INT32_MAX);
  if (n == "phrase_boost") return (int)std::min<int64_t>(st->rules.tally_phrase, INT32_MAX);
  if (n == "repeat_rule") return (int)std::min<int64_t>(st->rules.tally_repeat, INT32_MAX);
  if (n == "command_rule") return (int)std::min<int64_t>(st->rules.tally_command, INT32_MAX);
  if (n == "enc_rows") return (int)std::min<int64_t>(st->enc_rows, INT32_MAX);
  auto clamp = [](int64_t v) { return (int)std::min<int64_t>(v, INT32_MAX); };
  if (n == "token_score") return clamp(st->tally_score);
  if (n == "score_buffers") return st->sc_logits.p ? 1 : 0;
  if (n == "dec_gemm.total" || n == "xattn.total") {        // every launch of the family, whatever its variant
    int64_t t = 0;
    if (n[0] == 'd') for (int g = 0; g < DT_GEMMS; ++g) for (int f = 0; f < DT_FORMS; ++f) for (int k = 0; k < DG_N_SHAPES; ++k) t += st->tally_gemm[g][f][k];
    else for (int v = 0; v < XA_N_VARIANTS; ++v) t += st->tally_xattn[v];
    return clamp(t);
  }
  for (int g = 0; g < DT_GEMMS; ++g)
    for (int f = 0; f < DT_FORMS; ++f)
      for (int k = 0; k < DG_N_SHAPES; ++k)
        if (n == std::string("dec_gemm.") + kDecTallyGemm[g] + kDecTallyForm[f] + "." + kDecTallyShape[k]) return clamp(st->tally_gemm[g][f][k]);
  for (int v = 0; v < XA_N_VARIANTS; ++v)
    if (n == std::string("xattn.") + kXattnTally[v]) return clamp(st->tally_xattn[v]);
  for (int v = 0; v < 4; ++v)
    if (n == std::string("self_attn.") + kSelfAttnTally[v]) return clamp(st->tally_self[v]);
  return OHW_E_INVALID_ARG;
}

int ohw_state_set_persistent(ohw_state* st, int on) {
  if (!st) return OHW_E_INVALID_ARG;
  st->persist = on != 0;
  return OHW_OK;
}

int ohw_state_set_packed_encoder(ohw_state* st, int on) {
  if (!st) return OHW_E_INVALID_ARG;
  st->packed = on != 0;
  return OHW_OK;
}
int ohw_state_packed_encoder(const ohw_state* st) { return st ? (st->packed ? 1 : 0) : OHW_E_INVALID_ARG; }

int ohw_state_set_batch_invariant(ohw_state* st, int on) {
  if (!st) return OHW_E_INVALID_ARG;
  st->batch_invariant = on != 0;
  return OHW_OK;
}

int ohw_state_set_audio_ctx(ohw_state* st, int n_ctx) {
  return guard([&] {
    if (!st) throw Error(OHW_E_INVALID_ARG, "state is null");
    const int full = st->ctx->hp.n_audio_ctx;
    if (n_ctx < 0 || n_ctx > full) throw Error(OHW_E_INVALID_ARG, "audio_ctx must be in 0.." + std::to_string(full) + " (0 = full context)");
    st->audio_ctx = n_ctx == full ? 0 : n_ctx;
    st->win_ctx.clear();      // lengths are given inside an envelope: a new envelope starts without any
  });
}

int ohw_state_audio_ctx(const ohw_state* st) { return st ? audio_ctx_of(st) : OHW_E_INVALID_ARG; }

int ohw_state_set_window_ctx(ohw_state* st, const int32_t* n_ctx, int batch) {
  return guard([&] {
    if (!st) throw Error(OHW_E_INVALID_ARG, "state is null");
    if (!n_ctx || batch == 0) { st->win_ctx.clear(); return; }
    if (batch < 0 || batch > st->max_batch) throw Error(OHW_E_INVALID_ARG, "window_ctx: batch exceeds the state's max_batch");
    const int E = audio_ctx_of(st);
    for (int b = 0; b < batch; ++b)
      if (n_ctx[b] < 1 || n_ctx[b] > E)
        throw Error(OHW_E_INVALID_ARG, "window_ctx: window " + std::to_string(b) + " asks for " + std::to_string(n_ctx[b]) + " positions, the state's context is " +
                                           std::to_string(E) + " (1.." + std::to_string(E) + ")");
    HIP_CHECK(hipSetDevice(st->ctx->device));
    // in stream order behind the kernels that still read the previous lengths; the source is the caller's memory, so wait
    HIP_CHECK(hipMemcpyAsync(st->wc_enc.p, n_ctx, (size_t)batch * 4, hipMemcpyHostToDevice, st->stream));
    HIP_CHECK(hipStreamSynchronize(st->stream));
    st->win_ctx.assign(n_ctx, n_ctx + batch);
  });
}

int ohw_state_window_ctx(const ohw_state* st, int window) {
  if (!st || window < 0 || window >= st->max_batch) return OHW_E_INVALID_ARG;
  return st->enc_var && window < st->enc_batch ? st->enc_win[(size_t)window] : audio_ctx_of(st);
}

int ohw_state_set_window_lang(ohw_state* st, const int32_t* lang_ids, int batch) {
  return guard([&] {
    if (!st) throw Error(OHW_E_INVALID_ARG, "state is null");
    if (!lang_ids || batch == 0) { st->lang_kind.clear(); st->lang_ids.clear(); return; }
    const ohw_ctx* c = st->ctx;
    if (c->hp.n_vocab < 51865) throw Error(OHW_E_INVALID_ARG, "window_lang: an English-only model has no language token");
    if (batch < 0 || batch > st->max_batch) throw Error(OHW_E_INVALID_ARG, "window_lang: batch exceeds the state's max_batch");
    for (int b = 0; b < batch; ++b)
      if (lang_ids[b] != OHW_LANG_DETECT && (lang_ids[b] < 0 || lang_ids[b] >= c->tok.n_langs))
        throw Error(OHW_E_INVALID_ARG, "window_lang: window " + std::to_string(b) + " asks for language id " + std::to_string(lang_ids[b]) + " (0.." +
                                           std::to_string(c->tok.n_langs - 1) + ", or OHW_LANG_DETECT)");
    static_assert(OHW_LANG_DETECT == LANG_PENDING, "the table stores OHW_LANG_DETECT as it is given");
    HIP_CHECK(hipSetDevice(c->device));
    // in stream order behind the kernels that still read the previous table; the source is the caller's memory, so wait
    HIP_CHECK(hipMemcpyAsync(st->lang_tab.p, lang_ids, (size_t)batch * 4, hipMemcpyHostToDevice, st->stream));
    HIP_CHECK(hipStreamSynchronize(st->stream));
    st->lang_ids.assign(lang_ids, lang_ids + batch);
    st->lang_kind.resize((size_t)batch);
    for (int b = 0; b < batch; ++b) st->lang_kind[(size_t)b] = lang_ids[b] == OHW_LANG_DETECT ? ohw_state::LANG_WAITING : ohw_state::LANG_EXPLICIT;
  });
}

int ohw_state_set_window_prompt(ohw_state* st, const int32_t* tokens, int stride, const int32_t* n_tokens, int batch) {
  return guard([&] {
    if (!st) throw Error(OHW_E_INVALID_ARG, "state is null");
    if (!tokens || batch == 0) { st->wp_len.clear(); st->wp_host.clear(); return; }
    const ohw_ctx* c = st->ctx;
    const int C = c->hp.n_text_ctx, cap = C / 2 - 1;
    if (!n_tokens) throw Error(OHW_E_INVALID_ARG, "window_prompt: n_tokens is null");
    if (batch < 0 || batch > st->max_batch) throw Error(OHW_E_INVALID_ARG, "window_prompt: batch exceeds the state's max_batch");
    if (cap < 1 || (C / 2 + st->wp_chunk - 1) / st->wp_chunk * st->wp_chunk > C)
      throw Error(OHW_E_INVALID_ARG, "window_prompt: the model's text context is too short for a prompt");
    for (int b = 0; b < batch; ++b) {
      if (n_tokens[b] < 0 || n_tokens[b] > cap)
        throw Error(OHW_E_INVALID_ARG, "window_prompt: window " + std::to_string(b) + " has " + std::to_string(n_tokens[b]) + " context tokens (0.." +
                                           std::to_string(cap) + " = n_text_ctx / 2 - 1)");
      if (n_tokens[b] > stride) throw Error(OHW_E_INVALID_ARG, "window_prompt: window " + std::to_string(b) + " has more tokens than the stride");
      for (int i = 0; i < n_tokens[b]; ++i) {
        const int32_t t = tokens[(size_t)b * stride + i];
        if (t < 0 || t >= c->hp.n_vocab)
          throw Error(OHW_E_INVALID_ARG, "window_prompt: window " + std::to_string(b) + ", token " + std::to_string(i) + " = " + std::to_string(t) +
                                             " is outside 0.." + std::to_string(c->hp.n_vocab - 1));
      }
    }
    std::vector<std::vector<int32_t>> host((size_t)batch);
    for (int b = 0; b < batch; ++b) {
      if (n_tokens[b] == 0) continue;
      host[(size_t)b].push_back(c->tok.prev);
      host[(size_t)b].insert(host[(size_t)b].end(), tokens + (size_t)b * stride, tokens + (size_t)b * stride + n_tokens[b]);
    }
    window_prompt_upload(st, host);
    st->wp_host = std::move(host);
  });
}

int ohw_state_set_prefill_chunk(ohw_state* st, int positions) {
  return guard([&] {
    if (!st) throw Error(OHW_E_INVALID_ARG, "state is null");
    if (positions != 8 && positions != 16) throw Error(OHW_E_INVALID_ARG, "set_prefill_chunk: 8 or 16 positions, got " + std::to_string(positions));
    if (positions == st->wp_chunk) return;
    const int C = st->ctx->hp.n_text_ctx;
    if ((C / 2 + positions - 1) / positions * positions > C)
      throw Error(OHW_E_INVALID_ARG, "set_prefill_chunk: the model's text context is too short for chunks of " + std::to_string(positions));
    st->wp_chunk = positions;
    if (!st->wp_len.empty()) {
      try {
        window_prompt_upload(st, st->wp_host);
      } catch (...) {
        st->wp_chunk = positions == 8 ? 16 : 8;
        throw;
      }
    }
  });
}

int ohw_state_prefill_chunk(const ohw_state* st) { return st ? st->wp_chunk : OHW_E_INVALID_ARG; }

int ohw_state_window_prompt_len(const ohw_state* st, int window) {
  if (!st || window < 0 || window >= st->max_batch) return OHW_E_INVALID_ARG;
  return window < (int)st->wp_len.size() ? st->wp_len[(size_t)window] : 0;
}

int ohw_state_prefill(ohw_state* st, int batch, const int32_t* active) {
  return guard([&] {
    if (!st) throw Error(OHW_E_INVALID_ARG, "state is null");
    if (st->wp_len.empty()) return;
    if (batch < 1 || batch != st->enc_batch) throw Error(OHW_E_INVALID_ARG, "prefill: batch must equal the batch of the last ohw_encode");
    check_decode_ctx(st, "prefill");
    HIP_CHECK(hipSetDevice(st->ctx->device));
    run_prefill(st, batch, active, "prefill");
    persist_check(st);
  });
}

int ohw_state_detect_window_lang(ohw_state* st, int batch) {
  return guard([&] {
    if (!st) throw Error(OHW_E_INVALID_ARG, "state is null");
    if (st->lang_kind.empty()) throw Error(OHW_E_INVALID_ARG, "detect_window_lang: no language table is set (ohw_state_set_window_lang)");
    if (batch < 1 || batch != st->enc_batch) throw Error(OHW_E_INVALID_ARG, "detect_window_lang: batch must equal the batch of the last ohw_encode");
    if ((int)st->lang_kind.size() != batch)
      throw Error(OHW_E_INVALID_ARG, "detect_window_lang: ohw_state_set_window_lang named " + std::to_string(st->lang_kind.size()) + " windows, the batch has " +
                                         std::to_string(batch));
    check_decode_ctx(st, "detect_window_lang");
    bool waiting = false;
    for (int8_t k : st->lang_kind) waiting = waiting || k == ohw_state::LANG_WAITING;
    if (!waiting) return;
    const ohw_ctx* c = st->ctx;
    HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = st->stream;
    // the step of ohw_detect_language: [sot] at position 0 for every window of the batch
    const std::vector<int32_t> toks((size_t)batch, c->tok.sot);
    HIP_CHECK(hipMemcpyAsync(st->step_tok.p, toks.data(), toks.size() * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemsetAsync(st->n_past.p, 0, (size_t)batch * 4, s));
    Dispatch::run(c->dtype, [&](auto* tag) {
      using T = std::remove_pointer_t<decltype(tag)>;
      run_decoder_step<T>(st, batch, 1);
    });
    launch_lang_pick(st->logits.as<float>(), st->logits_ld, c->tok.sot, c->tok.n_langs, st->lang_tab.as<int32_t>(), st->lang_prob.as<float>(), batch, s);
    HIP_CHECK(hipStreamSynchronize(s));     // toks is a stack-lifetime source
    persist_check(st);
    for (auto& k : st->lang_kind)
      if (k == ohw_state::LANG_WAITING) k = ohw_state::LANG_RESOLVED;
  });
}

int ohw_state_window_lang(ohw_state* st, int batch, int32_t* ids_out, float* probs_out) {
  return guard([&] {
    if (!st || !ids_out) throw Error(OHW_E_INVALID_ARG, "null argument");
    if (st->lang_kind.empty()) throw Error(OHW_E_INVALID_ARG, "window_lang: no language table is set (ohw_state_set_window_lang)");
    if (batch != (int)st->lang_kind.size()) throw Error(OHW_E_INVALID_ARG, "window_lang: batch must equal the batch of ohw_state_set_window_lang");
    const int nl = st->ctx->tok.n_langs;
    HIP_CHECK(hipSetDevice(st->ctx->device));
    hipStream_t s = st->stream;
    HIP_CHECK(hipMemcpyAsync(ids_out, st->lang_tab.p, (size_t)batch * 4, hipMemcpyDeviceToHost, s));
    if (probs_out) HIP_CHECK(hipMemcpyAsync(probs_out, st->lang_prob.p, (size_t)batch * nl * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (!probs_out) return;
    for (int b = 0; b < batch; ++b) {
      if (st->lang_kind[(size_t)b] == ohw_state::LANG_RESOLVED) continue;
      float* row = probs_out + (size_t)b * nl;
      std::fill(row, row + nl, 0.f);
      if (st->lang_kind[(size_t)b] == ohw_state::LANG_EXPLICIT) row[ids_out[b]] = 1.f;
    }
  });
}

// test entry: the device language pick on caller-supplied rows, logits [batch][n_vocab] (host), with a table of its own
int ohw_dbg_lang_pick(ohw_state* st, const float* logits, int batch, int32_t* ids_out, float* probs_out) {
  return guard([&] {
    if (!st || !logits || !ids_out) throw Error(OHW_E_INVALID_ARG, "null argument");
    if (batch < 1 || batch > st->max_batch) throw Error(OHW_E_INVALID_ARG, "dbg_lang_pick: batch exceeds the state's max_batch");
    const ohw_ctx* c = st->ctx;
    const int V = c->hp.n_vocab, nl = c->tok.n_langs;
    if (V < 51865) throw Error(OHW_E_INVALID_ARG, "dbg_lang_pick: an English-only model has no language tokens");
    HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = st->stream;
    DevBuf tab, prob;
    tab.alloc((size_t)batch * 4);
    prob.alloc((size_t)batch * nl * 4);       // the kernel writes every element of a pending row
    const std::vector<int32_t> pending((size_t)batch, LANG_PENDING);
    HIP_CHECK(hipMemcpyAsync(tab.p, pending.data(), pending.size() * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpy2DAsync(st->logits.p, (size_t)st->logits_ld * 4, logits, (size_t)V * 4, (size_t)V * 4, (size_t)batch, hipMemcpyHostToDevice, s));
    launch_lang_pick(st->logits.as<float>(), st->logits_ld, c->tok.sot, nl, tab.as<int32_t>(), prob.as<float>(), batch, s);
    HIP_CHECK(hipMemcpyAsync(ids_out, tab.p, (size_t)batch * 4, hipMemcpyDeviceToHost, s));
    if (probs_out) HIP_CHECK(hipMemcpyAsync(probs_out, prob.p, (size_t)batch * nl * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  });
}

int32_t ohw_audio_ctx_for(int64_t n_samples) {
  if (n_samples < 0) n_samples = 0;
  const int64_t pos = (n_samples + 319) / 320 + 32;      // 320 samples per encoder position, 0.64 s of headroom
  return (int32_t)std::min<int64_t>(1500, (pos + 63) / 64 * 64);
}

// the four logit rules of a state: LogitRules (logit_rules.hpp) checks, builds and uploads; a setter waits for the state's stream
int ohw_state_set_logit_bias(ohw_state* st, const float* bias, int n) {
  return guard([&] {
    if (!st) throw Error(OHW_E_INVALID_ARG, "state is null");
    st->rules.set_bias(bias, n);
  });
}

int ohw_state_set_phrase_table(ohw_state* st, const int32_t* tokens, const int32_t* offsets, const float* boosts, int n_phrases) {
  return guard([&] {
    if (!st) throw Error(OHW_E_INVALID_ARG, "state is null");
    st->rules.set_phrases(tokens, offsets, boosts, n_phrases);
  });
}

int ohw_state_phrase_count(const ohw_state* st) { return st ? st->rules.phrase_count() : 0; }

int ohw_state_set_repeat_rule(ohw_state* st, float penalty, int ngram) {
  return guard([&] {
    repeat_rule_check(penalty, ngram);                 // the values first: a refusal needs no state and no device
    if (!st) throw Error(OHW_E_INVALID_ARG, "state is null");
    st->rules.set_repeat(penalty, ngram);
  });
}

int ohw_state_repeat_rule(const ohw_state* st, float* penalty, int* ngram) {
  if (!st || !penalty || !ngram) return OHW_E_INVALID_ARG;
  *penalty = st->rules.rp.penalty; *ngram = st->rules.rp.ngram;
  return OHW_OK;
}

int ohw_state_set_command_table(ohw_state* st, const int32_t* tokens, const int32_t* offsets, int n_phrases, float penalty) {
  return guard([&] {
    if (n_phrases != 0) command_penalty_check(penalty);  // the value first: a refusal needs no state and no device
    if (!st) throw Error(OHW_E_INVALID_ARG, "state is null");
    st->rules.set_commands(tokens, offsets, n_phrases, penalty);
  });
}

int ohw_state_command_count(const ohw_state* st) { return st ? st->rules.command_count() : 0; }

int ohw_state_command_list_logprob(ohw_state* st, int batch, float* out) {
  return guard([&] {
    if (!st || !out) throw Error(OHW_E_INVALID_ARG, "null argument");
    st->rules.list_logprob(batch, out);
  });
}

// test entry: phrase_boost_kernel once on caller data: one history, length and flag per launch row
int ohw_dbg_phrase_boost(ohw_state* st, float* logits, int rows, int64_t ld, int n_vocab, const int32_t* histories, int max_tokens,
                         const int32_t* n_cur, const int32_t* done, const ohw_phrase_table* table) {
  return guard([&] {
    if (!st || !logits || !histories || !n_cur || !done || !table) throw Error(OHW_E_INVALID_ARG, "null argument");
    LogitRules own;
    dbg_rule_rows(st, "dbg_phrase_boost", {logits, rows, ld, n_vocab, histories, max_tokens, n_cur, done, rows, 1, 1, 0}, 65536, INT32_MAX,
                  [&] { own.upload_phrases(table, n_vocab); },         // checks the table's every count and child token
                  [&](float* d_logits, const int32_t* d_hist, const int32_t* d_ncur, const int32_t* d_done, hipStream_t s) {
                    PhraseBoostParams b{};
                    b.logits = d_logits; b.ld = ld; b.n_vocab = n_vocab; b.max_tokens = max_tokens; b.row_mul = 1; b.group = 1;
                    b.tokens = d_hist; b.n_cur = d_ncur; b.done = d_done; b.table = own.ph.table.as<int32_t>();
                    launch_phrase_boost(b, rows, s);
                  });
  });
}

// test entry: repeat_rule_kernel once on caller data
int ohw_dbg_repeat_rule(ohw_state* st, float* logits, int rows, int64_t ld, int n_vocab, const int32_t* histories, int max_tokens,
                        const int32_t* n_cur, const int32_t* done, int n_entries, int row_mul, int group, float penalty, int ngram, int eot) {
  return guard([&] {
    repeat_rule_check(penalty, ngram);
    if (!st || !logits || !histories || !done) throw Error(OHW_E_INVALID_ARG, "null argument");
    LogitRules own;
    dbg_rule_rows(st, "dbg_repeat_rule", {logits, rows, ld, n_vocab, histories, max_tokens, n_cur, done, n_entries, row_mul, group, eot}, 4096, INT32_MAX,
                  [&] { own.upload_repeat(penalty, ngram); },
                  [&](float* d_logits, const int32_t* d_hist, const int32_t* d_ncur, const int32_t* d_done, hipStream_t s) {
                    RepeatRuleParams q{};
                    q.logits = d_logits; q.ld = ld; q.n_vocab = n_vocab; q.max_tokens = max_tokens; q.row_mul = row_mul; q.group = group; q.eot = eot;
                    q.tokens = d_hist; q.n_cur = d_ncur; q.done = d_done; q.rule = own.rp.rule.as<int32_t>();
                    launch_repeat_rule(q, rows, s);
                  });
  });
}

// test entry: command_rule_kernel once on caller data; list_logprob [n_entries] goes in and comes back like the logits
int ohw_dbg_command_rule(ohw_state* st, float* logits, int rows, int64_t ld, int n_vocab, const int32_t* histories, int max_tokens,
                         const int32_t* n_cur, const int32_t* done, int n_entries, int row_mul, int group, float penalty, int eot,
                         const ohw_command_table* table, float* list_logprob) {
  return guard([&] {
    command_penalty_check(penalty);
    if (!st || !logits || !histories || !done || !table || !list_logprob) throw Error(OHW_E_INVALID_ARG, "null argument");
    LogitRules own;
    own.max_batch = std::max(n_entries, 0);              // its list_logprob buffer holds the caller's entries
    dbg_rule_rows(st, "dbg_command_rule", {logits, rows, ld, n_vocab, histories, max_tokens, n_cur, done, n_entries, row_mul, group, eot}, 4096, CM_MAX_VOCAB,
                  [&] { own.upload_commands(table, penalty); },        // checks the table's every count and index
                  [&](float* d_logits, const int32_t* d_hist, const int32_t* d_ncur, const int32_t* d_done, hipStream_t s) {
                    float* d_lp = own.cm.lp.as<float>();
                    HIP_CHECK(hipMemcpyAsync(d_lp, list_logprob, (size_t)n_entries * 4, hipMemcpyHostToDevice, s));
                    CommandRuleParams q{};
                    q.logits = d_logits; q.ld = ld; q.n_vocab = n_vocab; q.max_tokens = max_tokens; q.row_mul = row_mul; q.group = group; q.lp_group = group;
                    q.eot = eot; q.tokens = d_hist; q.n_cur = d_ncur; q.done = d_done; q.table = own.cm.table.as<int32_t>(); q.list_logprob = d_lp;
                    launch_command_rule(q, rows, s);
                    HIP_CHECK(hipMemcpyAsync(list_logprob, d_lp, (size_t)n_entries * 4, hipMemcpyDeviceToHost, s));
                  });
  });
}

// test entry: the device sampler on caller-supplied rows.  logits [batch][n_vocab] (host), history [batch][hist_stride]
// with n_hist[b] tokens sampled so far.  Returns the token the sampler picks per row (end-of-text included), its
// log-probability, and the first-step no-speech probability (rows with n_hist == 0; 0 elsewhere).
// temperature > 0: the temperature sampler, uniforms [batch] the draw of each row's step
static void dbg_sample(ohw_state* st, const ohw_sample_params* sp, const float* logits, const int32_t* history, int hist_stride,
                       const int32_t* n_hist, int batch, float temperature, const double* uniforms, int32_t* tokens_out, float* logprobs_out,
                       float* no_speech_out) {
    if (!st || !sp || !logits || !n_hist || !tokens_out) throw Error(OHW_E_INVALID_ARG, "null argument");
    if (temperature > 0.0f && !uniforms) throw Error(OHW_E_INVALID_ARG, "dbg_sample_t: uniforms is null");
    if (batch < 1 || batch > st->max_batch) throw Error(OHW_E_INVALID_ARG, "dbg_sample: batch exceeds the state's max_batch");
    const ohw_ctx* c = st->ctx;
    const int V = c->hp.n_vocab;
    HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = st->stream;
    std::vector<int32_t> hist((size_t)batch * st->max_tokens, 0), ncur((size_t)batch);
    for (int b = 0; b < batch; ++b) {
      if (n_hist[b] < 0 || n_hist[b] >= st->max_tokens || n_hist[b] > hist_stride || (n_hist[b] > 0 && !history))
        throw Error(OHW_E_INVALID_ARG, "dbg_sample: bad history length");
      ncur[(size_t)b] = n_hist[b];
      for (int i = 0; i < n_hist[b]; ++i) hist[(size_t)b * st->max_tokens + i] = history[(size_t)b * hist_stride + i];
    }
    HIP_CHECK(hipMemcpy2DAsync(st->logits.p, (size_t)st->logits_ld * 4, logits, (size_t)V * 4, (size_t)V * 4, (size_t)batch, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->tokens.p, hist.data(), hist.size() * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->n_cur.p, ncur.data(), ncur.size() * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemsetAsync(st->n_past.p, 0, (size_t)batch * 4, s));
    HIP_CHECK(hipMemsetAsync(st->done.p, 0, (size_t)batch * 4, s));
    HIP_CHECK(hipMemsetAsync(st->n_done.p, 0, 16, s));
    HIP_CHECK(hipMemsetAsync(st->sum_lp.p, 0, (size_t)batch * 4, s));
    HIP_CHECK(hipMemsetAsync(st->next_tok.p, 0, (size_t)batch * 4, s));
    HIP_CHECK(hipMemsetAsync(st->nosp_prob.p, 0, (size_t)batch * 4, s));
    SamplerParams spar;
    fill_sampler(st, sp, batch, &spar);
    spar.advance = 0;
    std::vector<double> u;
    if (temperature > 0.0f) {
      u.assign((size_t)batch * st->max_tokens, 0.0);
      for (int b = 0; b < batch; ++b) u[(size_t)b * st->max_tokens + n_hist[b]] = uniforms[b];
      HIP_CHECK(hipMemcpyAsync(st->samp_temp.p, &temperature, 4, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemcpyAsync(st->samp_u.p, u.data(), u.size() * 8, hipMemcpyHostToDevice, s));
      launch_sampler_t(spar, st->samp_temp.as<float>(), st->samp_u.as<double>(), s);
    } else {
      launch_sampler(spar, s);
    }
    std::vector<float> lps((size_t)batch * (st->max_tokens + 1));
    HIP_CHECK(hipMemcpyAsync(tokens_out, st->next_tok.p, (size_t)batch * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(lps.data(), st->tok_lp.p, lps.size() * 4, hipMemcpyDeviceToHost, s));
    if (no_speech_out) HIP_CHECK(hipMemcpyAsync(no_speech_out, st->nosp_prob.p, (size_t)batch * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (logprobs_out)
      for (int b = 0; b < batch; ++b) logprobs_out[b] = lps[(size_t)b * (st->max_tokens + 1) + n_hist[b]];
}

int ohw_dbg_sample(ohw_state* st, const ohw_sample_params* sp, const float* logits, const int32_t* history, int hist_stride,
                   const int32_t* n_hist, int batch, int32_t* tokens_out, float* logprobs_out, float* no_speech_out) {
  return guard([&] { dbg_sample(st, sp, logits, history, hist_stride, n_hist, batch, 0.0f, nullptr, tokens_out, logprobs_out, no_speech_out); });
}

int ohw_dbg_sample_t(ohw_state* st, const ohw_sample_params* sp, const float* logits, const int32_t* history, int hist_stride,
                     const int32_t* n_hist, int batch, float temperature, const double* uniforms, int32_t* tokens_out, float* logprobs_out,
                     float* no_speech_out) {
  return guard([&] {
    if (!(temperature > 0.0f)) throw Error(OHW_E_INVALID_ARG, "dbg_sample_t: temperature must be > 0");
    dbg_sample(st, sp, logits, history, hist_stride, n_hist, batch, temperature, uniforms, tokens_out, logprobs_out, no_speech_out);
  });
}

// test entry: one sampler launch on caller-supplied rows and state, the whole output back (include/ohw.h).  Everything is
// range-checked first: the kernels index with these values
int ohw_dbg_sample_ex(ohw_state* st, const ohw_sample_params* sp, const ohw_dbg_sample_io* io) {
  return guard([&] {
    if (!st || !sp || !io) throw Error(OHW_E_INVALID_ARG, "null argument");
    if (!io->logits || !io->tokens || !io->n_cur || !io->n_past || !io->done || !io->sum_logprob || !io->next_tok || !io->tok_lp ||
        !io->nosp_prob || !io->n_done || !io->tickets_out)
      throw Error(OHW_E_INVALID_ARG, "dbg_sample_ex: null array");
    const ohw_ctx* c = st->ctx;
    const int B = io->batch, V = c->hp.n_vocab, MT = st->max_tokens, C = c->hp.n_text_ctx;
    const float T = io->temperature;
    if (B < 1 || B > st->max_batch) throw Error(OHW_E_INVALID_ARG, "dbg_sample_ex: batch must be in 1..max_batch");
    if (io->advance != 0 && io->advance != 1) throw Error(OHW_E_INVALID_ARG, "dbg_sample_ex: advance must be 0 or 1");
    if (!(T >= 0.0f) || T == INFINITY) throw Error(OHW_E_INVALID_ARG, "dbg_sample_ex: temperature must be finite and >= 0");
    if (T > 0.0f && !io->uniforms) throw Error(OHW_E_INVALID_ARG, "dbg_sample_ex: uniforms is null");
    for (int b = 0; b < B; ++b) {
      if (io->n_cur[b] < 0 || io->n_cur[b] >= MT) throw Error(OHW_E_INVALID_ARG, "dbg_sample_ex: n_cur out of range");
      if (io->n_past[b] < 0 || (int64_t)io->n_past[b] + io->advance >= C) throw Error(OHW_E_INVALID_ARG, "dbg_sample_ex: n_past out of range");
      for (int i = 0; i < io->n_cur[b]; ++i)
        if (io->tokens[(size_t)b * MT + i] < 0 || io->tokens[(size_t)b * MT + i] >= V) throw Error(OHW_E_INVALID_ARG, "dbg_sample_ex: history token out of range");
      if (T > 0.0f && !(io->uniforms[b] >= 0.0 && io->uniforms[b] < 1.0)) throw Error(OHW_E_INVALID_ARG, "dbg_sample_ex: a uniform outside [0, 1)");
    }
    HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = st->stream;
    std::vector<int32_t> hist(io->tokens, io->tokens + (size_t)B * MT), rdone((size_t)B);
    for (int b = 0; b < B; ++b) {
      hist[(size_t)b * MT + io->n_cur[b]] = OHW_DBG_SENTINEL_I32;
      rdone[(size_t)b] = io->done[b] ? 1 : 0;
    }
    const std::vector<int32_t> sent_i((size_t)B, OHW_DBG_SENTINEL_I32);
    const std::vector<float> sent_f((size_t)B * (MT + 1), OHW_DBG_SENTINEL_F32);
    HIP_CHECK(hipMemcpy2DAsync(st->logits.p, (size_t)st->logits_ld * 4, io->logits, (size_t)V * 4, (size_t)V * 4, (size_t)B, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->tokens.p, hist.data(), hist.size() * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->n_cur.p, io->n_cur, (size_t)B * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->n_past.p, io->n_past, (size_t)B * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->done.p, rdone.data(), (size_t)B * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->sum_lp.p, io->sum_logprob, (size_t)B * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->next_tok.p, sent_i.data(), (size_t)B * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->tok_lp.p, sent_f.data(), (size_t)B * (MT + 1) * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->nosp_prob.p, sent_f.data(), (size_t)B * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemsetAsync(st->n_done.p, 0, 16, s));
    SamplerParams spar;
    fill_sampler(st, sp, B, &spar);
    spar.advance = io->advance;
    std::vector<double> u;
    if (T > 0.0f) {
      u.assign((size_t)B * MT, 0.0);
      for (int b = 0; b < B; ++b) u[(size_t)b * MT + io->n_cur[b]] = io->uniforms[b];
      HIP_CHECK(hipMemcpyAsync(st->samp_temp.p, &T, 4, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemcpyAsync(st->samp_u.p, u.data(), u.size() * 8, hipMemcpyHostToDevice, s));
      launch_sampler_t(spar, st->samp_temp.as<float>(), st->samp_u.as<double>(), s);
    } else {
      launch_sampler(spar, s);
    }
    HIP_CHECK(hipMemcpyAsync(io->tokens, st->tokens.p, (size_t)B * MT * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(io->n_cur, st->n_cur.p, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(io->n_past, st->n_past.p, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(io->done, st->done.p, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(io->sum_logprob, st->sum_lp.p, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(io->next_tok, st->next_tok.p, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(io->tok_lp, st->tok_lp.p, (size_t)B * (MT + 1) * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(io->nosp_prob, st->nosp_prob.p, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(io->n_done, st->n_done.p, 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(io->tickets_out, st->samp_ticket.p, (size_t)B * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  });
}

// test entry: the group sampler of ohw_sample_pass_n once on caller-supplied rows (include/ohw.h)
int ohw_dbg_sample_group(ohw_state* st, const ohw_sample_params* sp, const float* logits, const int32_t* history, int hist_stride,
                         const int32_t* n_hist, int n_windows, int group, int first, float temperature, const double* uniforms,
                         int32_t* done, int32_t* tokens_out, float* logprobs_out, float* no_speech_out, int32_t* win_done_out,
                         int32_t* n_cur_out) {
  return guard([&] {
    if (!st || !sp || !logits || !n_hist || !uniforms || !done || !tokens_out || !win_done_out) throw Error(OHW_E_INVALID_ARG, "null argument");
    if (!(temperature > 0.0f)) throw Error(OHW_E_INVALID_ARG, "dbg_sample_group: temperature must be > 0");
    if (group < 1 || group > 5 || n_windows < 1) throw Error(OHW_E_INVALID_ARG, "dbg_sample_group: 1..5 candidates per window, at least one window");
    const int W = n_windows, R = W * group;
    if (R > st->max_batch) throw Error(OHW_E_INVALID_ARG, "dbg_sample_group: rows exceed the state's max_batch");
    const ohw_ctx* c = st->ctx;
    const int V = c->hp.n_vocab, MT = st->max_tokens, MB = st->max_batch;
    HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = st->stream;
    std::vector<int32_t> hist((size_t)R * MT, 0), ncur((size_t)R), wdone((size_t)W), rdone((size_t)R);
    std::vector<unsigned> wcnt((size_t)W, 0u);
    std::vector<double> u((size_t)R * MT, 0.0);
    for (int r = 0; r < R; ++r) {
      if (n_hist[r] < 0 || n_hist[r] >= MT || n_hist[r] > hist_stride || (n_hist[r] > 0 && !history)) throw Error(OHW_E_INVALID_ARG, "dbg_sample_group: bad history length");
      ncur[(size_t)r] = n_hist[r];
      for (int i = 0; i < n_hist[r]; ++i) hist[(size_t)r * MT + i] = history[(size_t)r * hist_stride + i];
      u[(size_t)r * MT + n_hist[r]] = uniforms[r];
      rdone[(size_t)r] = done[r] ? 1 : 0;
      wcnt[(size_t)(r / group)] += (unsigned)rdone[(size_t)r];
    }
    for (int w = 0; w < W; ++w) wdone[(size_t)w] = wcnt[(size_t)w] == (unsigned)group ? 1 : 0;
    if (!st->sn_slot.p) { st->sn_slot.alloc((size_t)MB * c->hp.n_text_ctx * 4, true); st->sn_win.alloc((size_t)MB * 4 * 4, true); }
    int32_t* d_wdone = st->sn_win.as<int32_t>() + 2 * MB;
    unsigned* d_wcnt = (unsigned*)(st->sn_win.as<int32_t>() + 3 * MB);
    HIP_CHECK(hipMemcpy2DAsync(st->logits.p, (size_t)st->logits_ld * 4, logits, (size_t)V * 4, (size_t)V * 4, (size_t)(first ? W : R), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->tokens.p, hist.data(), hist.size() * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->n_cur.p, ncur.data(), ncur.size() * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->done.p, rdone.data(), rdone.size() * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_wdone, wdone.data(), wdone.size() * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_wcnt, wcnt.data(), wcnt.size() * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemsetAsync(st->n_done.p, 0, 16, s));
    for (DevBuf* b : {&st->n_past, &st->sum_lp, &st->next_tok, &st->nosp_prob}) HIP_CHECK(hipMemsetAsync(b->p, 0, (size_t)R * 4, s));
    HIP_CHECK(hipMemsetAsync(st->tok_lp.p, 0, (size_t)R * (MT + 1) * 4, s));
    SamplerParams spar;
    fill_sampler(st, sp, R, &spar);
    spar.advance = first ? 0 : 1;
    HIP_CHECK(hipMemcpyAsync(st->samp_temp.p, &temperature, 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->samp_u.p, u.data(), u.size() * 8, hipMemcpyHostToDevice, s));
    launch_sampler_group(spar, SampGroup{group, d_wdone, d_wcnt}, st->samp_temp.as<float>(), st->samp_u.as<double>(), s);
    std::vector<float> lps((size_t)R * (MT + 1));
    HIP_CHECK(hipMemcpyAsync(tokens_out, st->next_tok.p, (size_t)R * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(lps.data(), st->tok_lp.p, lps.size() * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(done, st->done.p, (size_t)R * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(win_done_out, d_wdone, (size_t)W * 4, hipMemcpyDeviceToHost, s));
    if (n_cur_out) HIP_CHECK(hipMemcpyAsync(n_cur_out, st->n_cur.p, (size_t)R * 4, hipMemcpyDeviceToHost, s));
    if (no_speech_out) HIP_CHECK(hipMemcpyAsync(no_speech_out, st->nosp_prob.p, (size_t)R * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (logprobs_out)
      for (int r = 0; r < R; ++r) logprobs_out[r] = lps[(size_t)r * (MT + 1) + n_hist[r]];
  });
}

// test entry: one beam step on caller-supplied rows and state (include/ohw.h).  Everything is range-checked first: the
// kernels index with these values.
// x: the log-probability history and the no-speech probability of ohw_dbg_beam_step_ex, or null
static void dbg_beam_step_run(ohw_state* st, const ohw_sample_params* sp, const ohw_dbg_beam_io* io, const ohw_dbg_beam_io_ex* x) {
  {
    if (!st || !sp || !io) throw Error(OHW_E_INVALID_ARG, "null argument");
    const bool lp = x && x->plog;
    if (lp && (!x->plog_next || !x->fin_plog)) throw Error(OHW_E_INVALID_ARG, "dbg_beam_step_ex: plog needs plog_next and fin_plog");
    if (!io->logits || !io->tokens || !io->kv_slot || !io->n_cur || !io->n_past_w || !io->win_done || !io->beam_sum || !io->fin_cnt ||
        !io->fin_tok || !io->fin_len || !io->fin_sum || !io->cand_tok || !io->cand_lp || !io->tokens_next || !io->kv_slot_next ||
        !io->next_tok || !io->n_past || !io->n_done || !io->tickets_out)
      throw Error(OHW_E_INVALID_ARG, "dbg_beam_step: null array");
    const ohw_ctx* c = st->ctx;
    const int K = io->K, W = io->W, first = io->first != 0, q = io->side;
    const int V = c->hp.n_vocab, C = c->hp.n_text_ctx, MT = st->max_tokens;
    if (K < 2 || K > 5) throw Error(OHW_E_INVALID_ARG, "dbg_beam_step: K must be in 2..5");
    if (W < 1 || (int64_t)W * K > st->max_batch) throw Error(OHW_E_INVALID_ARG, "dbg_beam_step: W * K exceeds the state's max_batch");
    if (q != 0 && q != 1) throw Error(OHW_E_INVALID_ARG, "dbg_beam_step: side must be 0 or 1");
    if (sp->force_len > 0) throw Error(OHW_E_INVALID_ARG, "dbg_beam_step: force_len is a greedy-only knob");
    if (MT != C) throw Error(OHW_E_INVALID_ARG, "dbg_beam_step: the state's token capacity is not n_text_ctx");
    const int R = W * K, K1 = K + 1;
    for (int w = 0; w < W; ++w) {
      if (io->fin_cnt[w] < 0 || io->fin_cnt[w] > K) throw Error(OHW_E_INVALID_ARG, "dbg_beam_step: fin_cnt out of range");
      for (int f = 0; f < io->fin_cnt[w]; ++f)
        if (io->fin_len[w * K + f] < 0 || io->fin_len[w * K + f] > MT) throw Error(OHW_E_INVALID_ARG, "dbg_beam_step: fin_len out of range");
      // both kernels leave a finished window at once: its counters (which may stand at a limit) and rows are never read
      if (io->win_done[w]) continue;
      if (io->n_cur[w] < 0 || io->n_cur[w] >= MT) throw Error(OHW_E_INVALID_ARG, "dbg_beam_step: n_cur out of range");
      if (io->n_past_w[w] < 0 || io->n_past_w[w] + 2 > C) throw Error(OHW_E_INVALID_ARG, "dbg_beam_step: n_past_w out of range");
      for (int j = 0; j < K; ++j) {
        const size_t r = (size_t)(w * K + j);
        for (int i = 0; i < io->n_cur[w]; ++i)
          if (io->tokens[r * MT + i] < 0 || io->tokens[r * MT + i] >= V) throw Error(OHW_E_INVALID_ARG, "dbg_beam_step: history token out of range");
        if (!first)
          for (int i = 0; i <= io->n_past_w[w]; ++i)
            if (io->kv_slot[r * C + i] < 0 || io->kv_slot[r * C + i] >= R) throw Error(OHW_E_INVALID_ARG, "dbg_beam_step: kv_slot entry out of range");
      }
    }
    HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = st->stream;
    alloc_beam_buffers(st);
    int32_t* tokbuf[2] = {st->tokens.as<int32_t>(), st->bm_tok2.as<int32_t>()};
    // inputs; the pool slots from fin_cnt[w] on hold the sentinel
    std::vector<int32_t> fin_tok(io->fin_tok, io->fin_tok + (size_t)R * MT), fin_len(io->fin_len, io->fin_len + R);
    std::vector<float> fin_sum(io->fin_sum, io->fin_sum + R);
    for (int w = 0; w < W; ++w)
      for (int f = io->fin_cnt[w]; f < K; ++f) {
        std::fill_n(&fin_tok[(size_t)(w * K + f) * MT], (size_t)MT, OHW_DBG_SENTINEL_I32);
        fin_len[(size_t)(w * K + f)] = OHW_DBG_SENTINEL_I32;
        fin_sum[(size_t)(w * K + f)] = OHW_DBG_SENTINEL_F32;
      }
    const std::vector<int32_t> sent_i((size_t)R * std::max(MT, C), OHW_DBG_SENTINEL_I32);
    const std::vector<float> sent_f((size_t)R * K1, OHW_DBG_SENTINEL_F32);
    HIP_CHECK(hipMemcpy2DAsync(st->logits.p, (size_t)st->logits_ld * 4, io->logits, (size_t)V * 4, (size_t)V * 4, (size_t)(first ? W : R), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(tokbuf[q], io->tokens, (size_t)R * MT * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(tokbuf[q ^ 1], sent_i.data(), (size_t)R * MT * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->bm_slot[q].p, io->kv_slot, (size_t)R * C * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->bm_slot[q ^ 1].p, sent_i.data(), (size_t)R * C * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->bm_cand_tok.p, sent_i.data(), (size_t)R * K1 * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->bm_cand_lp.p, sent_f.data(), (size_t)R * K1 * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->next_tok.p, sent_i.data(), (size_t)R * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->n_past.p, sent_i.data(), (size_t)R * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->bm_ncur.p, io->n_cur, (size_t)W * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->bm_npast.p, io->n_past_w, (size_t)W * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->bm_done.p, io->win_done, (size_t)W * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->bm_sum.p, io->beam_sum, (size_t)R * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->bm_fin_cnt.p, io->fin_cnt, (size_t)W * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->bm_fin_tok.p, fin_tok.data(), (size_t)R * MT * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->bm_fin_len.p, fin_len.data(), (size_t)R * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->bm_fin_sum.p, fin_sum.data(), (size_t)R * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemsetAsync(st->n_done.p, 0, 16, s));
    std::vector<float> fin_plog;
    const std::vector<float> sent_lp(lp ? (size_t)R * (MT + 1) : (size_t)W, OHW_DBG_SENTINEL_F32);
    if (lp) {
      fin_plog.assign(x->fin_plog, x->fin_plog + (size_t)R * (MT + 1));
      for (int w = 0; w < W; ++w)
        for (int f = io->fin_cnt[w]; f < K; ++f) std::fill_n(&fin_plog[(size_t)(w * K + f) * (MT + 1)], (size_t)MT + 1, OHW_DBG_SENTINEL_F32);
      HIP_CHECK(hipMemcpyAsync(st->bm_plog[q].p, x->plog, (size_t)R * (MT + 1) * 4, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemcpyAsync(st->bm_plog[q ^ 1].p, sent_lp.data(), (size_t)R * (MT + 1) * 4, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemcpyAsync(st->bm_fin_plog.p, fin_plog.data(), (size_t)R * (MT + 1) * 4, hipMemcpyHostToDevice, s));
    }
    if (x && x->nosp_prob) HIP_CHECK(hipMemcpyAsync(st->bm_nosp.p, sent_lp.data(), (size_t)W * 4, hipMemcpyHostToDevice, s));
    SamplerParams p;
    fill_sampler(st, sp, R, &p);
    p.tokens = tokbuf[q];
    BeamParams bp = beam_params(st, K, q, lp, 1);
    if (x && x->nosp_prob) bp.nosp_prob = st->bm_nosp.as<float>();
    launch_beam_step(p, bp, W, first, s);
    if (lp) {
      HIP_CHECK(hipMemcpyAsync(x->plog_next, st->bm_plog[q ^ 1].p, (size_t)R * (MT + 1) * 4, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipMemcpyAsync(x->fin_plog, st->bm_fin_plog.p, (size_t)R * (MT + 1) * 4, hipMemcpyDeviceToHost, s));
    }
    if (x && x->nosp_prob) HIP_CHECK(hipMemcpyAsync(x->nosp_prob, st->bm_nosp.p, (size_t)W * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(io->cand_tok, st->bm_cand_tok.p, (size_t)R * K1 * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(io->cand_lp, st->bm_cand_lp.p, (size_t)R * K1 * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(io->tokens_next, tokbuf[q ^ 1], (size_t)R * MT * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(io->kv_slot_next, st->bm_slot[q ^ 1].p, (size_t)R * C * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(io->next_tok, st->next_tok.p, (size_t)R * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(io->n_past, st->n_past.p, (size_t)R * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(io->n_done, st->n_done.p, 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(io->tickets_out, st->bm_ticket.p, (size_t)R * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(io->n_cur, st->bm_ncur.p, (size_t)W * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(io->n_past_w, st->bm_npast.p, (size_t)W * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(io->win_done, st->bm_done.p, (size_t)W * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(io->beam_sum, st->bm_sum.p, (size_t)R * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(io->fin_cnt, st->bm_fin_cnt.p, (size_t)W * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(io->fin_tok, st->bm_fin_tok.p, (size_t)R * MT * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(io->fin_len, st->bm_fin_len.p, (size_t)R * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(io->fin_sum, st->bm_fin_sum.p, (size_t)R * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  }
}
int ohw_dbg_beam_step(ohw_state* st, const ohw_sample_params* sp, const ohw_dbg_beam_io* io) {
  return guard([&] { dbg_beam_step_run(st, sp, io, nullptr); });
}
int ohw_dbg_beam_step_ex(ohw_state* st, const ohw_sample_params* sp, const ohw_dbg_beam_io_ex* io) {
  return guard([&] {
    if (!io) throw Error(OHW_E_INVALID_ARG, "null argument");
    dbg_beam_step_run(st, sp, &io->base, io);
  });
}

// the range checks of the two finish entries: the ranking indexes with these values
static void check_beam_finish_io(const ohw_beam_finish_io* io) {
  if (!io) throw Error(OHW_E_INVALID_ARG, "null argument");
  if (!io->fin_cnt || !io->fin_len || !io->fin_sum || !io->fin_tok || !io->fin_plog || !io->n_cur || !io->tokens || !io->plog || !io->beam_sum ||
      !io->out_tokens || !io->out_logprobs || !io->n_tokens || !io->sum_logprob || !io->ended_by_eot || !io->n_finished)
    throw Error(OHW_E_INVALID_ARG, "beam finish: null array");
  const int K = io->K, W = io->W;
  if (K < 2 || K > 5 || W < 1) throw Error(OHW_E_INVALID_ARG, "beam finish: K must be in 2..5 and W >= 1");
  if (io->stride < 1 || io->max_tokens < 0 || io->max_tokens > io->stride) throw Error(OHW_E_INVALID_ARG, "beam finish: need 1 <= stride and 0 <= max_tokens <= stride");
  for (int w = 0; w < W; ++w) {
    if (io->fin_cnt[w] < 0 || io->fin_cnt[w] > K) throw Error(OHW_E_INVALID_ARG, "beam finish: fin_cnt out of range");
    for (int f = 0; f < io->fin_cnt[w]; ++f)
      if (io->fin_len[w * K + f] < 0 || io->fin_len[w * K + f] > io->stride) throw Error(OHW_E_INVALID_ARG, "beam finish: fin_len out of range");
    if (io->n_cur[w] < 0 || io->n_cur[w] > io->stride) throw Error(OHW_E_INVALID_ARG, "beam finish: n_cur out of range");
  }
}
static void fill_beam_finish_out(const ohw_beam_finish_io* io) {
  const size_t W = (size_t)io->W, n = (size_t)io->max_tokens;
  std::fill_n(io->out_tokens, W * n, OHW_DBG_SENTINEL_I32); std::fill_n(io->out_logprobs, W * (n + 1), OHW_DBG_SENTINEL_F32);
  std::fill_n(io->n_tokens, W, OHW_DBG_SENTINEL_I32); std::fill_n(io->sum_logprob, W, OHW_DBG_SENTINEL_F32);
  std::fill_n(io->ended_by_eot, W, OHW_DBG_SENTINEL_I32); std::fill_n(io->n_finished, W, OHW_DBG_SENTINEL_I32);
}

int ohw_beam_finish_host(const ohw_beam_finish_io* io) {
  return guard([&] {
    check_beam_finish_io(io);
    fill_beam_finish_out(io);
    // the rule writes rows of the input's stride; the caller's rows are max_tokens (+ 1) long
    const size_t W = (size_t)io->W, S = (size_t)io->stride, n = (size_t)io->max_tokens;
    std::vector<int32_t> tok(W * S, OHW_DBG_SENTINEL_I32);
    std::vector<float> lp(W * (S + 1), OHW_DBG_SENTINEL_F32);
    BeamFinishParams f{};
    f.K = io->K; f.stride = io->stride; f.max_tokens = io->max_tokens;
    f.fin_cnt = io->fin_cnt; f.fin_len = io->fin_len; f.fin_tok = io->fin_tok; f.n_cur = io->n_cur; f.tokens = io->tokens;
    f.fin_sum = io->fin_sum; f.fin_plog = io->fin_plog; f.beam_sum = io->beam_sum; f.plog = io->plog;
    f.out_tok = tok.data(); f.out_n = io->n_tokens; f.out_eot = io->ended_by_eot; f.out_nfin = io->n_finished; f.out_lp = lp.data(); f.out_sum = io->sum_logprob;
    beam_finish_host(f, io->W);
    for (size_t w = 0; w < W; ++w) {
      std::copy_n(&tok[w * S], n, io->out_tokens + w * n);
      std::copy_n(&lp[w * (S + 1)], n + 1, io->out_logprobs + w * (n + 1));
    }
  });
}

int ohw_dbg_beam_finish(ohw_state* st, const ohw_beam_finish_io* io) {
  return guard([&] {
    if (!st) throw Error(OHW_E_INVALID_ARG, "state is null");
    check_beam_finish_io(io);
    const int K = io->K, W = io->W, R = W * K, MT = st->max_tokens;
    if ((int64_t)W * K > st->max_batch) throw Error(OHW_E_INVALID_ARG, "dbg_beam_finish: W * K exceeds the state's max_batch");
    if (io->stride != MT) throw Error(OHW_E_INVALID_ARG, "dbg_beam_finish: stride must be the state's token capacity");
    fill_beam_finish_out(io);
    HIP_CHECK(hipSetDevice(st->ctx->device));
    hipStream_t s = st->stream;
    alloc_beam_buffers(st);
    const std::vector<int32_t> sent_i((size_t)W * MT, OHW_DBG_SENTINEL_I32);
    const std::vector<float> sent_f((size_t)W * (MT + 1), OHW_DBG_SENTINEL_F32);
    HIP_CHECK(hipMemcpyAsync(st->bm_fin_cnt.p, io->fin_cnt, (size_t)W * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->bm_fin_len.p, io->fin_len, (size_t)R * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->bm_fin_sum.p, io->fin_sum, (size_t)R * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->bm_fin_tok.p, io->fin_tok, (size_t)R * MT * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->bm_fin_plog.p, io->fin_plog, (size_t)R * (MT + 1) * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->bm_ncur.p, io->n_cur, (size_t)W * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->tokens.p, io->tokens, (size_t)R * MT * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->bm_plog[0].p, io->plog, (size_t)R * (MT + 1) * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->bm_sum.p, io->beam_sum, (size_t)R * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->bm_out_tok.p, sent_i.data(), (size_t)W * MT * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->bm_out_lp.p, sent_f.data(), (size_t)W * (MT + 1) * 4, hipMemcpyHostToDevice, s));
    for (DevBuf* b : {&st->bm_out_n, &st->bm_out_eot, &st->bm_out_nfin}) HIP_CHECK(hipMemcpyAsync(b->p, sent_i.data(), (size_t)W * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(st->bm_out_sum.p, sent_f.data(), (size_t)W * 4, hipMemcpyHostToDevice, s));
    launch_beam_finish(finish_params(st, K, io->max_tokens, 0), W, s);
    const size_t n = (size_t)io->max_tokens;
    if (n) HIP_CHECK(hipMemcpy2DAsync(io->out_tokens, n * 4, st->bm_out_tok.p, (size_t)MT * 4, n * 4, (size_t)W, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpy2DAsync(io->out_logprobs, (n + 1) * 4, st->bm_out_lp.p, (size_t)(MT + 1) * 4, (n + 1) * 4, (size_t)W, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(io->n_tokens, st->bm_out_n.p, (size_t)W * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(io->sum_logprob, st->bm_out_sum.p, (size_t)W * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(io->ended_by_eot, st->bm_out_eot.p, (size_t)W * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(io->n_finished, st->bm_out_nfin.p, (size_t)W * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  });
}

// ---- word timestamps (include/ohw.h; kernels in align.hip) ---------------------------------------------------------------
int ohw_state_set_align_heads(ohw_state* st, const ohw_align_head* heads, int n) {
  return guard([&] {
    if (!st) throw Error(OHW_E_INVALID_ARG, "state is null");
    const ohw_hparams& hp = st->ctx->hp;
    HIP_CHECK(hipSetDevice(st->ctx->device));
    if (n < 0) throw Error(OHW_E_INVALID_ARG, "set_align_heads: n < 0");
    if (n > OHW_ALIGN_MAX_HEADS)
      throw Error(OHW_E_INVALID_ARG, "set_align_heads: " + std::to_string(n) + " heads, at most " + std::to_string(OHW_ALIGN_MAX_HEADS) + " (OHW_ALIGN_MAX_HEADS)");
    if (heads)
      for (int i = 0; i < n; ++i)
        if (heads[i].layer < 0 || heads[i].layer >= hp.n_text_layer || heads[i].head < 0 || heads[i].head >= hp.n_text_head)
          throw Error(OHW_E_INVALID_ARG, "set_align_heads: entry " + std::to_string(i) + " (layer " + std::to_string(heads[i].layer) + ", head " +
                                             std::to_string(heads[i].head) + ") is outside the model (" + std::to_string(hp.n_text_layer) + " layers, " +
                                             std::to_string(hp.n_text_head) + " heads)");
    HIP_CHECK(hipStreamSynchronize(st->stream));
    st->al_batch = 0;
    if (!heads || n == 0) {
      st->al_heads.clear();
      for (DevBuf* b : {&st->al_p, &st->al_q, &st->al_stats, &st->al_m, &st->al_trace, &st->al_idx, &st->al_cnt, &st->al_tok}) b->release();
      return;
    }
    if ((size_t)n != st->al_heads.size() || !st->al_p.p) {
      const size_t B = (size_t)st->max_batch, A = (size_t)n, T = (size_t)hp.n_audio_ctx, half = (size_t)hp.n_text_ctx / 2;
      st->al_rows = (int)half + 8;
      st->al_p.alloc(B * A * (half + 8) * T * 4);
      st->al_q.alloc(B * (half + 8) * A * 64 * 4);
      st->al_stats.alloc(B * A * T * 2 * 4);
      st->al_m.alloc(B * (half + 1) * T * 4);
      st->al_trace.alloc(B * (half + 2) * (T + 1));
      st->al_idx.alloc(B * (half + 1) * 4, true);
      st->al_cnt.alloc(3 * B * 4, true);
      st->al_tok.alloc(((half + 8) / 8 + 1) * B * 8 * 4);
    }
    st->al_heads.assign(heads, heads + n);
  });
}

// the buffers of ohw_state_score; rows: 0 frees them, 1 makes them, 2 also the kept rows of "score_logits"
static void score_buffers(ohw_state* st, int mode) {
  if (mode == 0) {
    for (DevBuf* b : {&st->sc_logits, &st->sc_tok, &st->sc_tgt, &st->sc_cnt, &st->sc_out, &st->sc_keep}) b->release();
    st->sc_keep_rows = false;
    st->sc_batch = 0;
    return;
  }
  const size_t B = (size_t)st->max_batch, half = (size_t)st->ctx->hp.n_text_ctx / 2, chunks = (half + 8) / 8 + 1;
  if (!st->sc_logits.p) {
    st->sc_logits.alloc(B * 8 * (size_t)st->logits_ld * 4);
    st->sc_tok.alloc(chunks * B * 8 * 4);
    st->sc_tgt.alloc(chunks * B * 8 * 4);
    st->sc_cnt.alloc(B * 4, true);
    st->sc_out.alloc(B * (half + 1) * sizeof(ohw_token_score));
  }
  if (mode == 2 && !st->sc_keep.p) st->sc_keep.alloc(chunks * 8 * (size_t)st->logits_ld * 4);
  if (mode == 2) st->sc_keep_rows = true;
}

// The teacher-forced replay ohw_state_align and ohw_state_score share: the windows' sequences through the decoder in chunks of 8
// positions on the resident cross K/V.  start_idx_out: the tap runs behind the listed heads' cross-query GEMMs and the reduction
// and the DTW follow; scores_out: the logits GEMM keeps every row of a chunk and token_score_kernel reduces them behind each
// step.  what: "align" or "score", the name the refusals carry
static void replay_tokens(ohw_state* st, const ohw_sample_params* sp, const int32_t* tokens, int stride, const int32_t* n_tokens, const int32_t* n_frames,
                          int batch, int32_t* start_idx_out, ohw_token_score* scores_out, const std::string& what) {
  {
    const bool do_align = start_idx_out != nullptr, do_score = scores_out != nullptr;
    if (!st || !sp || !tokens || !n_tokens || (do_align && !n_frames) || (!do_align && !do_score)) throw Error(OHW_E_INVALID_ARG, what + ": null argument");
    if (do_align && st->al_heads.empty()) throw Error(OHW_E_INVALID_ARG, what + ": no alignment heads are set (ohw_state_set_align_heads)");
    if (batch < 1 || batch != st->enc_batch) throw Error(OHW_E_INVALID_ARG, what + ": batch must equal the batch of the last ohw_encode");
    check_decode_ctx(st, what.c_str());
    const ohw_ctx* c = st->ctx;
    const ohw_hparams& hp = c->hp;
    const bool multilingual = hp.n_vocab >= 51865, lang_tab = !st->lang_kind.empty();
    if (lang_tab) check_window_lang(st, batch, what);
    else if (multilingual && (sp->lang_id < 0 || sp->lang_id >= c->tok.n_langs)) throw Error(OHW_E_INVALID_ARG, what + ": lang_id out of range");
    const int half = hp.n_text_ctx / 2, eot = c->tok.eot;
    if (stride < 0) throw Error(OHW_E_INVALID_ARG, what + ": stride < 0");
    for (int b = 0; b < batch; ++b) {
      const int nt = n_tokens[b];
      if (nt < 0 || nt > stride || nt > half)
        throw Error(OHW_E_INVALID_ARG, what + ": window " + std::to_string(b) + " has n_tokens " + std::to_string(nt) + ", outside 0 .. min(stride " +
                                           std::to_string(stride) + ", n_text_ctx / 2 = " + std::to_string(half) + ")");
      if (do_align && n_frames[b] < 0) throw Error(OHW_E_INVALID_ARG, what + ": window " + std::to_string(b) + " has n_frames < 0");
      for (int k = 0; k < nt; ++k) {
        const int32_t id = tokens[(size_t)b * stride + k];
        if (id < 0 || id >= eot)
          throw Error(OHW_E_INVALID_ARG, what + ": window " + std::to_string(b) + ", token " + std::to_string(k) + ": id " + std::to_string(id) +
                                             " is not a text token (0 .. " + std::to_string(eot - 1) + ")");
      }
    }
    HIP_CHECK(hipSetDevice(c->device));
    hipStream_t s = st->stream;
    // the windows' language tokens: the table's ids (one read-back), else the caller's
    std::vector<int32_t> lang((size_t)batch, sp->lang_id);
    if (lang_tab && multilingual) {
      HIP_CHECK(hipMemcpyAsync(lang.data(), st->lang_tab.p, (size_t)batch * 4, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
    }
    const int P = 1 + (multilingual ? 2 : 0) + 1;
    const int MB = st->max_batch, Tn = st->enc_ctx;
    std::vector<int32_t> cnt((size_t)3 * MB, 0);      // n_all, n_keys, N
    int max_all = 0, max_nk = 1;
    for (int b = 0; b < batch; ++b) {
      const int nt = n_tokens[b];
      const int ctx_b = st->enc_var ? st->enc_win[(size_t)b] : Tn;
      const int nk = std::max(1, std::min(ctx_b, do_align ? n_frames[b] / 2 : ctx_b));
      cnt[(size_t)b] = nt > 0 ? P + nt + 1 : 0;
      cnt[(size_t)MB + b] = nk;
      cnt[(size_t)2 * MB + b] = nt > 0 ? nt + 1 : 0;
      max_all = std::max(max_all, cnt[(size_t)b]);
      if (nt > 0) max_nk = std::max(max_nk, nk);
    }
    const int chunks = (max_all + 7) / 8;
    if (chunks * 8 > hp.n_text_ctx || (do_align && (chunks * 8 > st->al_rows + 7 || (size_t)chunks * batch * 8 * 4 > st->al_tok.bytes)) ||
        (do_score && chunks > (half + 8) / 8 + 1))
      throw Error(OHW_E_INVALID_ARG, what + ": the sequence does not fit n_text_ctx");
    // nothing below refuses: from here on the "align_*" fetches describe this call (a failed launch ends their validity)
    if (do_align) {
      st->al_batch = 0;
      st->al_nall.assign(cnt.begin(), cnt.begin() + batch);
      st->al_nk.assign(cnt.begin() + MB, cnt.begin() + MB + batch);
      st->al_prompt = P;
    }
    if (do_score) {
      st->sc_batch = 0;
      score_buffers(st, st->sc_keep_rows ? 2 : 1);
    }
    if (max_all == 0) {     // every window skipped
      if (do_align) st->al_batch = batch;
      return;
    }
    // the score's own tables: positions with a score (the end-of-text INPUT position of the alignment has none), and per
    // row the token its position predicts
    std::vector<int32_t> sc_cnt((size_t)(do_score ? batch : 0)), tgt((size_t)(do_score ? chunks * batch * 8 : 0), eot);
    std::vector<int32_t> toks((size_t)chunks * batch * 8, eot), npast((size_t)chunks * batch);
    for (int b = 0; b < batch; ++b) {
      const int nt = n_tokens[b];
      if (nt == 0) continue;
      std::vector<int32_t> seq;
      seq.push_back(c->tok.sot);
      if (multilingual) { seq.push_back(c->tok.sot + 1 + lang[(size_t)b]); seq.push_back(sp->translate ? c->tok.translate : c->tok.transcribe); }
      seq.push_back(c->tok.no_timestamps);
      seq.insert(seq.end(), tokens + (size_t)b * stride, tokens + (size_t)b * stride + nt);
      for (size_t i = 0; i < seq.size(); ++i) toks[((i / 8) * batch + b) * 8 + i % 8] = seq[i];       // the tail stays eot
      if (do_score) {
        sc_cnt[(size_t)b] = P + nt;
        for (size_t i = 0; i + 1 < seq.size(); ++i) tgt[((i / 8) * batch + b) * 8 + i % 8] = seq[i + 1];   // the last position's stays eot
      }
    }
    for (int ch = 0; ch < chunks; ++ch)
      for (int b = 0; b < batch; ++b) npast[(size_t)ch * batch + b] = ch * 8;
    DevBuf& tok_buf = do_score ? st->sc_tok : st->al_tok;
    HIP_CHECK(hipMemcpyAsync(tok_buf.p, toks.data(), toks.size() * 4, hipMemcpyHostToDevice, s));
    if (do_align) HIP_CHECK(hipMemcpyAsync(st->al_cnt.p, cnt.data(), cnt.size() * 4, hipMemcpyHostToDevice, s));
    if (do_score) {
      HIP_CHECK(hipMemcpyAsync(st->sc_tgt.p, tgt.data(), tgt.size() * 4, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemcpyAsync(st->sc_cnt.p, sc_cnt.data(), sc_cnt.size() * 4, hipMemcpyHostToDevice, s));
    }
    {
      // the replay: launch-per-kernel steps only, every window's cross-attention runs, nothing is captured
      struct Replay {
        ohw_state* st; bool persist, fuse, skip;
        Replay(ohw_state* s_, bool tap, bool score) : st(s_), persist(s_->persist), fuse(s_->fuse_attn), skip(s_->skip_done) {
          st->persist = false; st->fuse_attn = false; st->skip_done = false; st->al_tap = tap; st->sc_on = score;
        }
        ~Replay() { st->persist = persist; st->fuse_attn = fuse; st->skip_done = skip; st->al_tap = false; st->sc_on = false; }
      } replay(st, do_align, do_score);
      st->al_lds = max_nk;
      TokenScoreParams tp{};
      tp.logits = st->sc_logits.as<float>(); tp.ld = st->logits_ld; tp.n_all = st->sc_cnt.as<int32_t>(); tp.n_prompt = P;
      tp.n_vocab = hp.n_vocab; tp.eot = eot; tp.batch = batch; tp.cap = half + 1; tp.out = st->sc_out.as<ohw_token_score>();
      Dispatch::run(c->dtype, [&](auto* tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        for (int ch = 0; ch < chunks; ++ch) {
          HIP_CHECK(hipMemcpyAsync(st->n_past.p, &npast[(size_t)ch * batch], (size_t)batch * 4, hipMemcpyHostToDevice, s));
          st->al_row0 = ch * 8;
          run_decoder_step<T>(st, batch, 8, tok_buf.as<int32_t>() + (size_t)ch * batch * 8);
          if (!do_score) continue;
          tp.row0 = ch * 8; tp.targets = st->sc_tgt.as<int32_t>() + (size_t)ch * batch * 8;
          launch_token_score(tp, s);
          ++st->tally_score;
          if (st->sc_keep_rows)
            HIP_CHECK(hipMemcpyAsync(st->sc_keep.as<float>() + (size_t)ch * 8 * st->logits_ld, st->sc_logits.as<float>() + (size_t)(batch - 1) * 8 * st->logits_ld,
                                     (size_t)8 * st->logits_ld * 4, hipMemcpyDeviceToDevice, s));
        }
      });
    }
    std::vector<ohw_token_score> sc_host((size_t)(do_score ? batch * (half + 1) : 0));
    if (do_score) HIP_CHECK(hipMemcpyAsync(sc_host.data(), st->sc_out.p, sc_host.size() * sizeof(ohw_token_score), hipMemcpyDeviceToHost, s));
    auto scores_back = [&] {
      for (int b = 0; do_score && b < batch; ++b)
        if (n_tokens[b] > 0) std::memcpy(scores_out + (size_t)b * (stride + 1), &sc_host[(size_t)b * (half + 1)], (size_t)(n_tokens[b] + 1) * sizeof(ohw_token_score));
      if (do_score) { st->sc_batch = batch; st->sc_chunks = chunks; }
    };
    if (!do_align) {
      HIP_CHECK(hipStreamSynchronize(s));     // also keeps toks / tgt / npast alive until their copies have run
      scores_back();
      return;
    }
    const int A = (int)st->al_heads.size();
    const int64_t T = hp.n_audio_ctx;
    AlignReduceParams rp{};
    rp.p = st->al_p.as<float>(); rp.p_row = T; rp.p_head = (int64_t)st->al_rows * T; rp.p_win = (int64_t)A * rp.p_head;
    rp.stats = st->al_stats.as<float>(); rp.ld_stat = T; rp.n_heads = A; rp.n_prompt = P; rp.max_rows = half + 1; rp.max_keys = Tn;
    rp.n_all = st->al_cnt.as<int32_t>(); rp.n_keys = st->al_cnt.as<int32_t>() + MB;
    rp.m = st->al_m.as<float>(); rp.m_row = T; rp.m_win = (int64_t)(half + 1) * T;
    launch_align_reduce(rp, batch, s);
    AlignDtwParams dp{};
    dp.m = rp.m; dp.m_win = rp.m_win; dp.m_row = rp.m_row; dp.n_rows = st->al_cnt.as<int32_t>() + 2 * MB; dp.n_keys = rp.n_keys;
    dp.trace = st->al_trace.as<uint8_t>(); dp.trace_win = (int64_t)(half + 2) * (T + 1); dp.idx = st->al_idx.as<int32_t>(); dp.idx_win = half + 1;
    dp.max_rows = half + 1; dp.max_keys = Tn;
    launch_align_dtw(dp, batch, s);
    std::vector<int32_t> idx((size_t)batch * (half + 1));
    HIP_CHECK(hipMemcpyAsync(idx.data(), st->al_idx.p, idx.size() * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));     // also keeps toks / cnt / npast alive until their copies have run
    st->al_batch = batch;
    for (int b = 0; b < batch; ++b)
      if (n_tokens[b] > 0) std::memcpy(start_idx_out + (size_t)b * (stride + 1), &idx[(size_t)b * (half + 1)], (size_t)(n_tokens[b] + 1) * 4);
    scores_back();
  }
}

int ohw_state_align(ohw_state* st, const ohw_sample_params* sp, const int32_t* tokens, int stride, const int32_t* n_tokens, const int32_t* n_frames,
                    int batch, int32_t* start_idx_out) {
  return guard([&] {
    if (!n_frames || !start_idx_out) throw Error(OHW_E_INVALID_ARG, "align: null argument");
    replay_tokens(st, sp, tokens, stride, n_tokens, n_frames, batch, start_idx_out, nullptr, "align");
  });
}

int ohw_state_score(ohw_state* st, const ohw_sample_params* sp, const int32_t* tokens, int stride, const int32_t* n_tokens, int batch,
                    ohw_token_score* scores_out, const int32_t* n_frames, int32_t* start_idx_out) {
  return guard([&] {
    if (!scores_out) throw Error(OHW_E_INVALID_ARG, "score: null argument");
    replay_tokens(st, sp, tokens, stride, n_tokens, n_frames, batch, start_idx_out, scores_out, "score");
  });
}

int ohw_state_set_score_buffers(ohw_state* st, int on) {
  return guard([&] {
    if (!st) throw Error(OHW_E_INVALID_ARG, "state is null");
    if (on < 0 || on > 2) throw Error(OHW_E_INVALID_ARG, "set_score_buffers: on must be 0 (free), 1 (make) or 2 (make, and keep the rows of \"score_logits\")");
    HIP_CHECK(hipSetDevice(st->ctx->device));
    HIP_CHECK(hipStreamSynchronize(st->stream));
    if (on != 2) st->sc_keep_rows = false;
    if (on != 2) st->sc_keep.release();
    score_buffers(st, on);
  });
}

int ohw_state_timings(ohw_state* st, ohw_timings* t) {
  return guard([&] {
    if (!st || !t) throw Error(OHW_E_INVALID_ARG, "null argument");
    HIP_CHECK(hipSetDevice(st->ctx->device));
    HIP_CHECK(hipStreamSynchronize(st->stream));
    auto el = [&](int a, int b) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, st->ev[a], st->ev[b]) != hipSuccess) ms = 0.f;
      return ms;
    };
    st->last.mel_ms = el(0, 1);
    st->last.encode_ms = el(2, 3);
    st->last.decode_ms = el(4, 5);
    st->last.total_ms = st->last.mel_ms + st->last.encode_ms + st->last.decode_ms;
    *t = st->last;
  });
}

int ohw_state_profile_begin(ohw_state* st, int kernel_class) {
  return guard([&] {
    if (!st) throw Error(OHW_E_INVALID_ARG, "state is null");
    if (kernel_class < 0 || kernel_class > 8) throw Error(OHW_E_INVALID_ARG, "unknown kernel class");
    HIP_CHECK(hipSetDevice(st->ctx->device));
    st->prof_class = kernel_class;
    st->prof_used = 0;
    st->prof_work = 0.0;
  });
}

int ohw_state_profile_end(ohw_state* st, int64_t* launches, double* total_ms, double* work) {
  return guard([&] {
    if (!st) throw Error(OHW_E_INVALID_ARG, "state is null");
    HIP_CHECK(hipSetDevice(st->ctx->device));
    HIP_CHECK(hipStreamSynchronize(st->stream));
    double ms = 0.0;
    for (size_t i = 0; i + 1 < st->prof_used; i += 2) {
      float t = 0.f;
      HIP_CHECK(hipEventElapsedTime(&t, st->prof_ev[i], st->prof_ev[i + 1]));
      ms += t;
    }
    if (launches) *launches = (int64_t)(st->prof_used / 2);
    if (total_ms) *total_ms = ms;
    if (work) *work = st->prof_work;
    st->prof_class = 0;
    st->prof_used = 0;
  });
}

int ohw_state_fetch(ohw_state* st, const char* what, int batch, float* out, int64_t out_elems) {
  return guard([&] {
    if (!st || !what || !out) throw Error(OHW_E_INVALID_ARG, "null argument");
    const ohw_hparams& hp = st->ctx->hp;
    HIP_CHECK(hipSetDevice(st->ctx->device));
    hipStream_t s = st->stream;
    if (std::string(what) == "sample_slots") {      // rows, not windows: n_windows * best_of of the last ohw_sample_pass_n
      if (st->sn_rows < 1 || batch != st->sn_rows) throw Error(OHW_E_INVALID_ARG, "fetch: sample_slots holds the " + std::to_string(st->sn_rows) + " rows of the last ohw_sample_pass_n");
      const int64_t n = (int64_t)batch * hp.n_text_ctx;
      if (out_elems < n) throw Error(OHW_E_INVALID_ARG, "fetch: output buffer too small");
      std::vector<int32_t> tab((size_t)n);
      HIP_CHECK(hipMemcpyAsync(tab.data(), st->sn_slot.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      for (int64_t i = 0; i < n; ++i) out[i] = (float)tab[(size_t)i];
      return;
    }
    if (std::string(what) == "logits") {            // decoder rows, not windows: the first `batch` rows as the last step and its sampler left them
      if (batch < 1 || batch > st->max_batch) throw Error(OHW_E_INVALID_ARG, "fetch: logits holds at most max_batch rows");
      if (out_elems < (int64_t)batch * hp.n_vocab) throw Error(OHW_E_INVALID_ARG, "fetch: output buffer too small");
      HIP_CHECK(hipMemcpy2DAsync(out, (size_t)hp.n_vocab * 4, st->logits.p, (size_t)st->logits_ld * 4, (size_t)hp.n_vocab * 4, (size_t)batch, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      return;
    }
    if (batch < 1 || batch > st->enc_batch) throw Error(OHW_E_INVALID_ARG, "fetch: batch exceeds the last encode");
    const int64_t d = hp.n_audio_state, Tn = st->enc_ctx;   // rows per window of the last encode
    const std::string w = what;
    DevBuf tmp;
    auto need = [&](int64_t n) { if (out_elems < n) throw Error(OHW_E_INVALID_ARG, "fetch: output buffer too small"); };
    auto from_t = [&](const void* src, int64_t n) {
      need(n);
      tmp.alloc((size_t)n * 4);
      Dispatch::run(st->ctx->dtype, [&](auto* tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        launch_to_f32<T>(src, tmp.as<float>(), n, s);
      });
      HIP_CHECK(hipMemcpyAsync(out, tmp.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
    };
    auto from_f32 = [&](const void* src, int64_t n) {
      need(n);
      HIP_CHECK(hipMemcpyAsync(out, src, (size_t)n * 4, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
    };
    if (w == "mel") { from_f32(st->logmel.p, (int64_t)batch * hp.n_mels * CHUNK_FRAMES); return; }
    if (w == "mel_t") { from_t(st->mel_t.p, (int64_t)batch * MEL_ROWS * MEL_CPAD); return; }   // the image conv1 reads, pad rows and channels included
    if (w == "score_logits") {
      // window batch - 1 of the last ohw_state_score: the call's last window, whose rows ohw_state_set_score_buffers(st, 2) keeps
      if (!st->sc_keep_rows || !st->sc_keep.p || st->sc_batch < 1 || batch != st->sc_batch)
        throw Error(OHW_E_INVALID_ARG, "fetch: score_logits holds window batch - 1 of the last ohw_state_score, under ohw_state_set_score_buffers(st, 2)");
      const int64_t rows = (int64_t)st->sc_chunks * 8;
      need(rows * hp.n_vocab);
      HIP_CHECK(hipMemcpy2DAsync(out, (size_t)hp.n_vocab * 4, st->sc_keep.p, (size_t)st->logits_ld * 4, (size_t)hp.n_vocab * 4, (size_t)rows, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      return;
    }
    if (w == "align_q" || w == "align_p" || w == "align_m") {
      // window batch - 1 of the last ohw_state_align
      const int b = batch - 1;
      if (st->al_heads.empty() || batch > st->al_batch || st->al_nall[(size_t)b] == 0)
        throw Error(OHW_E_INVALID_ARG, "fetch: window " + std::to_string(b) + " was not aligned by the last ohw_state_align");
      const int64_t A = (int64_t)st->al_heads.size(), n_all = st->al_nall[(size_t)b], nk = st->al_nk[(size_t)b], R = st->al_rows, T = hp.n_audio_ctx;
      const int64_t n_m = n_all - st->al_prompt, half = hp.n_text_ctx / 2;
      if (w == "align_q") { from_f32(st->al_q.as<float>() + (int64_t)b * R * A * 64, n_all * A * 64); return; }
      if (w == "align_p") {
        need(A * n_all * nk);
        for (int64_t a = 0; a < A; ++a)
          HIP_CHECK(hipMemcpy2DAsync(out + a * n_all * nk, (size_t)nk * 4, st->al_p.as<float>() + ((int64_t)b * A + a) * R * T, (size_t)T * 4, (size_t)nk * 4,
                                     (size_t)n_all, hipMemcpyDeviceToHost, s));
      } else {
        need(n_m * nk);
        HIP_CHECK(hipMemcpy2DAsync(out, (size_t)nk * 4, st->al_m.as<float>() + (int64_t)b * (half + 1) * T, (size_t)T * 4, (size_t)nk * 4, (size_t)n_m,
                                   hipMemcpyDeviceToHost, s));
      }
      HIP_CHECK(hipStreamSynchronize(s));
      return;
    }
    // the last encode ran packed: "enc" and "block0" lie end to end on the device; the caller gets the envelope layout [B][Tn][d],
    // window b's first n_ctx[b] rows from its packed rows, the rows behind them as zeros
    DevBuf unp;
    auto unpacked = [&](const void* src, int es) -> const void* {
      if (st->enc_pk.empty()) return src;
      unp.alloc((size_t)batch * Tn * d * es);
      HIP_CHECK(hipMemsetAsync(unp.p, 0, unp.bytes, s));
      for (int b = 0; b < batch && b < (int)st->enc_pk.size(); ++b)
        HIP_CHECK(hipMemcpyAsync((char*)unp.p + (size_t)b * Tn * d * es, (const char*)src + (size_t)st->enc_pk[(size_t)b] * d * es,
                                 (size_t)st->enc_set[(size_t)b] * d * es, hipMemcpyDeviceToDevice, s));
      return unp.p;
    };
    if (w == "enc") { from_t(unpacked(st->enc.p, 2), (int64_t)batch * Tn * d); return; }
    if (w == "stem" || w == "block0") {
      if (!st->taps) throw Error(OHW_E_INVALID_ARG, "fetch: taps are kept only for d_model <= 512");
      from_f32(w == "stem" ? st->tap_stem.p : unpacked(st->tap_block0.p, 4), (int64_t)batch * Tn * d);
      return;
    }
    if (w == "conv1") {
      // image rows 1..3000 of every window
      need((int64_t)batch * CHUNK_FRAMES * d);
      const int es = 2;
      tmp.alloc((size_t)batch * CHUNK_FRAMES * d * 4);
      DevBuf packed;
      packed.alloc((size_t)batch * CHUNK_FRAMES * d * es);
      for (int b = 0; b < batch; ++b)
        HIP_CHECK(hipMemcpyAsync((char*)packed.p + (size_t)b * CHUNK_FRAMES * d * es, (char*)st->c1.p + ((size_t)b * MEL_ROWS + 1) * d * es,
                                 (size_t)CHUNK_FRAMES * d * es, hipMemcpyDeviceToDevice, s));
      Dispatch::run(st->ctx->dtype, [&](auto* tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        launch_to_f32<T>(packed.p, tmp.as<float>(), (int64_t)batch * CHUNK_FRAMES * d, s);
      });
      HIP_CHECK(hipMemcpyAsync(out, tmp.p, (size_t)batch * CHUNK_FRAMES * d * 4, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      return;
    }
    if ((w.rfind("xk", 0) == 0 || w.rfind("xv", 0) == 0) && w.size() > 2) {
      // head-major [B][H][T][64] of layer l -> [B][T][d] on the host
      const int l = std::atoi(w.c_str() + 2);
      if (l < 0 || l >= hp.n_text_layer) throw Error(OHW_E_INVALID_ARG, "fetch: layer out of range");
      const int H = hp.n_text_head;
      const int64_t slab = (int64_t)st->enc_batch * H * Tn * 64;
      const int64_t n = (int64_t)batch * H * Tn * 64;
      need(n);
      std::vector<float> hm((size_t)n);
      tmp.alloc((size_t)n * 4);
      const int which = w[1] == 'k' ? 0 : 1;
      Dispatch::run(st->ctx->dtype, [&](auto* tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        launch_to_f32<T>((const T*)st->xkv.p + (int64_t)(2 * l + which) * slab, tmp.as<float>(), n, s);
      });
      HIP_CHECK(hipMemcpyAsync(hm.data(), tmp.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      for (int b = 0; b < batch; ++b)
        for (int h = 0; h < H; ++h)
          for (int64_t t = 0; t < Tn; ++t)
            std::memcpy(out + ((int64_t)b * Tn + t) * (H * 64) + h * 64, &hm[(size_t)((((int64_t)b * H + h) * Tn + t) * 64)], 64 * 4);
      return;
    }
    throw Error(OHW_E_INVALID_ARG, std::string("fetch: unknown activation '") + what + "'");
  });
}

int ohw_ctx_create_shell(const ohw_hparams* hp, int device, int dtype, ohw_ctx** out) {
  return guard([&] {
    if (!out) throw Error(OHW_E_INVALID_ARG, "out is null");
    *out = nullptr;
    *out = ctx_shell(hp, device, dtype);
  });
}

// blob = [weight arena | mel filterbank], each part padded to 256 bytes
static size_t blob_part(size_t n) { return (n + 255) / 256 * 256; }
size_t ohw_ctx_blob_size(const ohw_ctx* ctx) { return ctx ? blob_part(ctx->arena.bytes) + blob_part(ctx->mel_filters.bytes) : 0; }

int ohw_ctx_blob_export(const ohw_ctx* ctx, void* dst_device, size_t capacity) {
  return guard([&] {
    if (!ctx || !dst_device) throw Error(OHW_E_INVALID_ARG, "null argument");
    if (capacity < ohw_ctx_blob_size(ctx)) throw Error(OHW_E_INVALID_ARG, "blob_export: destination is smaller than ohw_ctx_blob_size");
    HIP_CHECK(hipSetDevice(ctx->device));
    HIP_CHECK(hipMemcpy(dst_device, ctx->arena.p, ctx->arena.bytes, hipMemcpyDeviceToDevice));
    HIP_CHECK(hipMemcpy((char*)dst_device + blob_part(ctx->arena.bytes), ctx->mel_filters.p, ctx->mel_filters.bytes, hipMemcpyDeviceToDevice));
    HIP_CHECK(hipDeviceSynchronize());
  });
}

int ohw_ctx_blob_import(ohw_ctx* ctx, const void* src_device, size_t bytes) {
  return guard([&] {
    if (!ctx || !src_device) throw Error(OHW_E_INVALID_ARG, "null argument");
    if (bytes != ohw_ctx_blob_size(ctx)) throw Error(OHW_E_LOAD_FAILED, "blob_import: size does not match this model's layout (hparams / dtype differ?)");
    HIP_CHECK(hipSetDevice(ctx->device));
    HIP_CHECK(hipMemcpy(ctx->arena.p, src_device, ctx->arena.bytes, hipMemcpyDeviceToDevice));
    HIP_CHECK(hipMemcpy(ctx->mel_filters.p, (const char*)src_device + blob_part(ctx->arena.bytes), ctx->mel_filters.bytes, hipMemcpyDeviceToDevice));
    HIP_CHECK(hipDeviceSynchronize());
  });
}

int ohw_ctx_weight_digest(const ohw_ctx* ctx, int index, char* name_out, uint64_t* digest) {
  return guard([&] {
    if (!ctx || !name_out || !digest || index < 0) throw Error(OHW_E_INVALID_ARG, "bad argument");
    std::vector<std::pair<std::string, const DevBuf*>> bufs;
    auto add = [&](const std::string& n, const DevBuf& b) { bufs.emplace_back(n, &b); };
    add("mel_filters", ctx->mel_filters); add("conv1_w", ctx->conv1_w); add("conv1_b", ctx->conv1_b);
    add("conv2_w", ctx->conv2_w); add("conv2_b", ctx->conv2_b); add("enc_pos", ctx->enc_pos);
    for (size_t i = 0; i < ctx->enc.size(); ++i) {
      const EncLayerW& l = ctx->enc[i];
      const std::string p = "enc" + std::to_string(i) + ".";
      add(p + "ln1.g", l.ln1.g); add(p + "ln1.b", l.ln1.b); add(p + "wqkv", l.wqkv); add(p + "bqkv", l.bqkv);
      add(p + "wo", l.wo); add(p + "bo", l.bo); add(p + "ln2.g", l.ln2.g); add(p + "ln2.b", l.ln2.b);
      add(p + "w1", l.w1); add(p + "b1", l.b1); add(p + "w2", l.w2); add(p + "b2", l.b2);
    }
    add("ln_post.g", ctx->ln_post.g); add("ln_post.b", ctx->ln_post.b); add("xkv_w", ctx->xkv_w); add("xkv_b", ctx->xkv_b);
    add("dec_pos", ctx->dec_pos); add("emb", ctx->emb);
    for (size_t i = 0; i < ctx->dec.size(); ++i) {
      const DecLayerW& l = ctx->dec[i];
      const std::string p = "dec" + std::to_string(i) + ".";
      add(p + "ln1.g", l.ln1.g); add(p + "ln1.b", l.ln1.b); add(p + "wqkv", l.wqkv); add(p + "bqkv", l.bqkv);
      add(p + "wo", l.wo); add(p + "bo", l.bo); add(p + "lnx.g", l.lnx.g); add(p + "lnx.b", l.lnx.b);
      add(p + "wxq", l.wxq); add(p + "bxq", l.bxq); add(p + "wxo", l.wxo); add(p + "bxo", l.bxo);
      add(p + "ln2.g", l.ln2.g); add(p + "ln2.b", l.ln2.b); add(p + "w1", l.w1); add(p + "b1", l.b1); add(p + "w2", l.w2); add(p + "b2", l.b2);
    }
    add("dec_ln.g", ctx->dec_ln.g); add("dec_ln.b", ctx->dec_ln.b);
    if ((size_t)index >= bufs.size()) throw Error(OHW_E_INVALID_ARG, "index past the last weight buffer");
    HIP_CHECK(hipSetDevice(ctx->device));
    const DevBuf& b = *bufs[(size_t)index].second;
    std::vector<unsigned char> host(b.bytes);
    HIP_CHECK(hipMemcpy(host.data(), b.p, b.bytes, hipMemcpyDeviceToHost));
    uint64_t h = 0xcbf29ce484222325ull;
    for (unsigned char c : host) { h ^= c; h *= 0x100000001b3ull; }
    *digest = h;
    std::snprintf(name_out, 64, "%s", bufs[(size_t)index].first.c_str());
  });
}

int ohw_dbg_gemm(int dtype, const void* A, const void* W, const float* bias, void* out, int64_t M, int64_t N, int64_t K, int epilogue,
                 void* stream) {
  return guard([&] {
    GemmParams g{};
    g.A = A; g.W = W; g.bias = bias; g.out = out; g.M = M; g.N = N; g.K = K;
    g.lda = K; g.a_batch_stride = 0; g.rows_per_batch = M; g.ldc = N; g.c_batch_stride = 0;
    if (epilogue != EPI_BIAS_T && epilogue != EPI_BIAS_GELU_T && epilogue != EPI_BIAS_RESID_F32 && epilogue != EPI_F32)
      throw Error(OHW_E_INVALID_ARG, "dbg_gemm: epilogue must be 0, 1, 2 or 4");
    Dispatch::run(dtype, [&](auto* tag) {
      using T = std::remove_pointer_t<decltype(tag)>;
      launch_gemm<T>(g, epilogue, (hipStream_t)stream);
    });
  });
}

int ohw_dbg_gemm_small(int dtype, const void* A, const void* W, const float* bias, void* out, int64_t M, int64_t N, int64_t K, int epilogue,
                       void* stream) {
  return guard([&] {
    GemmParams g{};
    g.A = A; g.W = W; g.bias = bias; g.out = out; g.M = M; g.N = N; g.K = K;
    g.lda = K; g.a_batch_stride = 0; g.rows_per_batch = M; g.ldc = N; g.c_batch_stride = 0;
    if (epilogue != EPI_BIAS_T && epilogue != EPI_BIAS_GELU_T && epilogue != EPI_BIAS_RESID_F32 && epilogue != EPI_F32)
      throw Error(OHW_E_INVALID_ARG, "dbg_gemm_small: epilogue must be 0, 1, 2 or 4");
    Dispatch::run(dtype, [&](auto* tag) {
      using T = std::remove_pointer_t<decltype(tag)>;
      launch_gemm_small<T>(g, epilogue, (hipStream_t)stream);
    });
  });
}

int ohw_dbg_dequantize(int device, int ttype, const void* blocks_host, int64_t n, float* out_host) {
  return guard([&] {
    const int bs = quant_block_bytes(ttype);
    if (bs == 0 || !blocks_host || !out_host || n <= 0 || n % QK != 0 || n > ((int64_t)1 << 31))
      throw Error(OHW_E_INVALID_ARG, "dbg_dequantize: ttype must be 2, 3, 6, 7 or 8 and n a positive multiple of 32 (at most 2^31)");
    select_device(device);
    const size_t raw_bytes = (size_t)(n / QK) * bs;
    DevBuf raw, out;
    raw.alloc(raw_bytes);
    out.alloc((size_t)n * 4);
    HIP_CHECK(hipMemcpy(raw.p, blocks_host, raw_bytes, hipMemcpyHostToDevice));
    launch_dequant_blocks(ttype, raw.p, out.as<float>(), n, nullptr);
    HIP_CHECK(hipStreamSynchronize(nullptr));
    HIP_CHECK(hipMemcpy(out_host, out.p, (size_t)n * 4, hipMemcpyDeviceToHost));
  });
}

int ohw_dbg_poison(ohw_state* st, const char* what) {
  return guard([&] {
    if (!st || !what) throw Error(OHW_E_INVALID_ARG, "null argument");
    const std::string w = what;
    const DevBuf* buf = w == "qkv" ? &st->qkv : w == "att" ? &st->att : nullptr;
    if (!buf) throw Error(OHW_E_INVALID_ARG, std::string("poison: unknown buffer '") + what + "'");
    HIP_CHECK(hipSetDevice(st->ctx->device));
    HIP_CHECK(hipMemsetAsync(buf->p, 0xff, buf->bytes, st->stream));
  });
}

int ohw_dbg_attention(int dtype, const void* qkv, void* out, int batch, int T, int n_head, void* stream) {
  return guard([&] {
    Dispatch::run(dtype, [&](auto* tag) {
      using TT = std::remove_pointer_t<decltype(tag)>;
      launch_encoder_attention<TT>(qkv, out, batch, T, n_head, (hipStream_t)stream);
    });
  });
}

// the small integer tables of the attention dbg entries arrive as host arrays: checked first, then copied to the device for
// the launch; the entry synchronises the stream before the copies are freed
static void dbg_upload(DevBuf& buf, const int32_t* host, size_t n) {
  buf.alloc(n * sizeof(int32_t));
  HIP_CHECK(hipMemcpy(buf.p, host, n * sizeof(int32_t), hipMemcpyHostToDevice));
}
static void dbg_check_dtype(int dtype, const char* what) {
  if (dtype != OHW_DTYPE_BF16 && dtype != OHW_DTYPE_F16) throw Error(OHW_E_INVALID_ARG, std::string(what) + ": dtype must be 0 (bf16) or 1 (f16)");
}

int ohw_dbg_attention_var(int dtype, const void* qkv, void* out, int batch, int T, int n_head, const int32_t* win_len_host,
                          const int32_t* win_off_host, void* stream) {
  return guard([&] {
    dbg_check_dtype(dtype, "dbg_attention_var");
    if (!qkv || !out || batch < 1 || T < 1 || n_head < 1) throw Error(OHW_E_INVALID_ARG, "dbg_attention_var: null buffer, or batch, T or n_head below 1");
    if (win_off_host && !win_len_host) throw Error(OHW_E_INVALID_ARG, "dbg_attention_var: packed rows (win_off) need the windows' lengths (win_len)");
    int64_t sum = 0;
    for (int b = 0; win_len_host && b < batch; ++b) {
      if (win_len_host[b] < 1 || win_len_host[b] > T)
        throw Error(OHW_E_INVALID_ARG, "dbg_attention_var: win_len[" + std::to_string(b) + "] = " + std::to_string(win_len_host[b]) + " is outside 1 .. T = " + std::to_string(T));
      if (win_off_host && win_off_host[b] != sum)
        throw Error(OHW_E_INVALID_ARG, "dbg_attention_var: win_off[" + std::to_string(b) + "] = " + std::to_string(win_off_host[b]) +
                                           " is not the exclusive prefix sum of win_len (" + std::to_string(sum) + ")");
      sum += win_len_host[b];
    }
    DevBuf len, off;
    if (win_len_host) dbg_upload(len, win_len_host, (size_t)batch);
    if (win_off_host) dbg_upload(off, win_off_host, (size_t)batch);
    Dispatch::run(dtype, [&](auto* tag) {
      using TT = std::remove_pointer_t<decltype(tag)>;
      launch_encoder_attention<TT>(qkv, out, batch, T, n_head, (hipStream_t)stream, win_len_host ? len.as<int32_t>() : nullptr,
                                   win_off_host ? off.as<int32_t>() : nullptr);
    });
    HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  });
}

int ohw_dbg_cross_attn(int dtype, const void* q, const void* xk, const void* xv, void* out, int M, int n_new, int n_head, int t_len,
                       int kv_group, int batch_invariant, const int32_t* done_host, const int32_t* win_len_host, float* partials,
                       unsigned* tickets, int max_split_rows, int* variant_out, void* stream) {
  return guard([&] {
    dbg_check_dtype(dtype, "dbg_cross_attn");
    if (!q || !xk || !xv || !out || M < 1 || n_new < 1 || n_head < 1 || t_len < 1)
      throw Error(OHW_E_INVALID_ARG, "dbg_cross_attn: null buffer, or M, n_new, n_head or t_len below 1");
    if (kv_group < 1 || kv_group > 5) throw Error(OHW_E_INVALID_ARG, "dbg_cross_attn: kv_group must be 1 .. 5 (beams per window)");
    if (kv_group > 1 && n_new != 1) throw Error(OHW_E_INVALID_ARG, "dbg_cross_attn: beams (kv_group > 1) are single-token rows: n_new must be 1");
    if (M % n_new != 0) throw Error(OHW_E_INVALID_ARG, "dbg_cross_attn: M must be a multiple of n_new");
    if (kv_group > 1 && M % kv_group != 0) throw Error(OHW_E_INVALID_ARG, "dbg_cross_attn: M must be a multiple of kv_group");
    if ((partials == nullptr) != (tickets == nullptr)) throw Error(OHW_E_INVALID_ARG, "dbg_cross_attn: partials and tickets come together");
    // a split form is picked only with scratch, without batch_invariant and without per-window lengths
    if (partials && !batch_invariant && !win_len_host && (max_split_rows < 1 || M > max_split_rows))
      throw Error(OHW_E_INVALID_ARG, "dbg_cross_attn: M = " + std::to_string(M) + " rows exceed max_split_rows = " + std::to_string(max_split_rows) +
                                         ", the rows the partials and tickets hold");
    const int windows = kv_group > 1 ? M / kv_group : M / n_new;
    for (int w = 0; win_len_host && w < windows; ++w)
      if (win_len_host[w] < 1 || win_len_host[w] > t_len)
        throw Error(OHW_E_INVALID_ARG, "dbg_cross_attn: win_len[" + std::to_string(w) + "] = " + std::to_string(win_len_host[w]) + " is outside 1 .. t_len = " + std::to_string(t_len));
    DevBuf done, len;
    if (done_host) dbg_upload(done, done_host, (size_t)windows);
    if (win_len_host) dbg_upload(len, win_len_host, (size_t)windows);
    int variant = -1;
    Dispatch::run(dtype, [&](auto* tag) {
      using TT = std::remove_pointer_t<decltype(tag)>;
      variant = launch_cross_attn<TT>(q, xk, xv, out, M, n_new, n_head, t_len, partials, tickets, max_split_rows,
                                      done_host ? done.as<int32_t>() : nullptr, (hipStream_t)stream, kv_group, batch_invariant != 0,
                                      win_len_host ? len.as<int32_t>() : nullptr);
    });
    HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    if (variant_out) *variant_out = variant;
  });
}

int ohw_dbg_cross_attn_chunk(int dtype, const void* q, const void* xk, const void* xv, void* out, int windows, int n_head, int t_len,
                             const int32_t* win_len_host, const int32_t* done_host, void* stream) {
  return ohw_dbg_cross_attn_chunk_n(dtype, q, xk, xv, out, windows, n_head, t_len, win_len_host, done_host, stream, 8);
}

int ohw_dbg_cross_attn_chunk_n(int dtype, const void* q, const void* xk, const void* xv, void* out, int windows, int n_head, int t_len,
                               const int32_t* win_len_host, const int32_t* done_host, void* stream, int n_q) {
  return guard([&] {
    dbg_check_dtype(dtype, "dbg_cross_attn_chunk");
    if (n_q != 8 && n_q != 16) throw Error(OHW_E_INVALID_ARG, "dbg_cross_attn_chunk: n_q is 8 or 16, got " + std::to_string(n_q));
    if (!q || !xk || !xv || !out || windows < 1 || n_head < 1 || t_len < 1)
      throw Error(OHW_E_INVALID_ARG, "dbg_cross_attn_chunk: null buffer, or windows, n_head or t_len below 1");
    for (int w = 0; win_len_host && w < windows; ++w)
      if (win_len_host[w] < 1 || win_len_host[w] > t_len)
        throw Error(OHW_E_INVALID_ARG, "dbg_cross_attn_chunk: win_len[" + std::to_string(w) + "] = " + std::to_string(win_len_host[w]) + " is outside 1 .. t_len = " + std::to_string(t_len));
    DevBuf done, len;
    if (done_host) dbg_upload(done, done_host, (size_t)windows);
    if (win_len_host) dbg_upload(len, win_len_host, (size_t)windows);
    Dispatch::run(dtype, [&](auto* tag) {
      using TT = std::remove_pointer_t<decltype(tag)>;
      launch_cross_attn_chunk<TT>(q, xk, xv, out, windows, n_head, t_len, done_host ? done.as<int32_t>() : nullptr,
                                  win_len_host ? len.as<int32_t>() : nullptr, (hipStream_t)stream, n_q);
    });
    HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  });
}

int ohw_dbg_self_attn(int dtype, const void* q, const void* k_cache, const void* v_cache, const int32_t* n_past_host, void* out, int M,
                      int n_new, int n_head, int n_ctx, const int32_t* kv_slot_host, int* variant_out, void* stream) {
  return guard([&] {
    dbg_check_dtype(dtype, "dbg_self_attn");
    if (!q || !k_cache || !v_cache || !n_past_host || !out || M < 1 || n_new < 1 || n_head < 1 || n_ctx < 1)
      throw Error(OHW_E_INVALID_ARG, "dbg_self_attn: null buffer, or M, n_new, n_head or n_ctx below 1");
    if (M % n_new != 0) throw Error(OHW_E_INVALID_ARG, "dbg_self_attn: M must be a multiple of n_new");
    const int rows = M / n_new;
    for (int b = 0; b < rows; ++b)
      if (n_past_host[b] < 0 || (int64_t)n_past_host[b] + n_new > n_ctx)
        throw Error(OHW_E_INVALID_ARG, "dbg_self_attn: n_past[" + std::to_string(b) + "] = " + std::to_string(n_past_host[b]) + " with n_new = " + std::to_string(n_new) +
                                           " is outside the " + std::to_string(n_ctx) + " positions of the cache");
    for (int64_t i = 0; kv_slot_host && i < (int64_t)rows * n_ctx; ++i)
      if (kv_slot_host[i] < 0 || kv_slot_host[i] >= rows)
        throw Error(OHW_E_INVALID_ARG, "dbg_self_attn: kv_slot[" + std::to_string(i / n_ctx) + "][" + std::to_string(i % n_ctx) + "] = " + std::to_string(kv_slot_host[i]) +
                                           " names no cache row (0 .. " + std::to_string(rows - 1) + ")");
    DevBuf past, slots;
    dbg_upload(past, n_past_host, (size_t)rows);
    if (kv_slot_host) dbg_upload(slots, kv_slot_host, (size_t)rows * n_ctx);
    int variant = -1;
    Dispatch::run(dtype, [&](auto* tag) {
      using TT = std::remove_pointer_t<decltype(tag)>;
      variant = launch_self_attn<TT>(q, k_cache, v_cache, past.as<int32_t>(), out, M, n_new, n_head, n_ctx, (hipStream_t)stream,
                                     kv_slot_host ? slots.as<int32_t>() : nullptr);
    });
    HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    if (variant_out) *variant_out = variant;
  });
}

static_assert(OHW_DEPI_QKV == DEPI_QKV && OHW_DEPI_BIAS_T == DEPI_BIAS_T && OHW_DEPI_BIAS_GELU_T == DEPI_BIAS_GELU_T &&
              OHW_DEPI_BIAS_RESID == DEPI_BIAS_RESID && OHW_DEPI_LOGITS == DEPI_LOGITS, "ohw.h names kernels.hpp's epilogues");
static_assert(OHW_DG_SHAPE_1x1 == DG_SHAPE_1x1 && OHW_DG_SHAPE_2x1 == DG_SHAPE_2x1 && OHW_DG_SHAPE_1x2 == DG_SHAPE_1x2 &&
              OHW_DG_SHAPE_2x2 == DG_SHAPE_2x2 && OHW_DG_SHAPE_4x2 == DG_SHAPE_4x2 && OHW_DG_SHAPE_1x6 == DG_SHAPE_1x6 &&
              OHW_DG_SHAPE_4x6 == DG_SHAPE_4x6 && OHW_DG_SHAPE_5x6 == DG_SHAPE_5x6, "ohw.h names kernels.hpp's shapes");

}  // extern "C"
// ohw_dbg_dec_gemm and ohw_dbg_logits_rows: one launch_dec_gemm on caller data; out_all (LOGITS only) may be null
static void dbg_dec_gemm_run(const ohw_dbg_dec_gemm_io* io, float* out_all, int64_t ld_all, void* stream) {
  {
    if (!io) throw Error(OHW_E_INVALID_ARG, "dbg_dec_gemm: null io");
    const ohw_dbg_dec_gemm_io& a = *io;
    auto bad = [](const std::string& why) { throw Error(OHW_E_INVALID_ARG, "dbg_dec_gemm: " + why); };
    dbg_check_dtype(a.dtype, "dbg_dec_gemm");
    if (a.epilogue < DEPI_QKV || a.epilogue > DEPI_LOGITS) bad("epilogue must be 0 .. 4");
    if (a.form < OHW_DG_FORM_PLAIN || a.form > OHW_DG_FORM_PN) bad("form must be 0 (plain), 1 (ln) or 2 (pn)");
    if (!a.w || !a.x || !a.out) bad("null w, x or out");
    if (a.M < 1 || a.N < 1 || a.K < 32 || a.M > (1 << 20) || a.N > (1 << 20) || a.K > (1 << 20)) bad("M, N >= 1 and K >= 32 (each at most 2^20)");
    if (a.K % 32 != 0) bad("K = " + std::to_string(a.K) + " must be a multiple of 32");
    if (a.cu_budget < 0 || a.ksplit < 0) bad("cu_budget and ksplit must not be negative");
    if ((a.gamma == nullptr) != (a.beta == nullptr)) bad("gamma and beta come together");
    const bool ln = a.form == OHW_DG_FORM_LN, pn = a.form == OHW_DG_FORM_PN;
    const bool t_epi = a.epilogue == DEPI_QKV || a.epilogue == DEPI_BIAS_T || a.epilogue == DEPI_BIAS_GELU_T;
    if ((ln || pn) && !t_epi) bad("the ln and pn forms exist for the QKV, BIAS_T and BIAS_GELU_T epilogues");
    if (ln && a.K > 1280) bad("ln: K = " + std::to_string(a.K) + " exceeds the 1280 columns of the fused LayerNorm");
    if (ln && a.K % 64 != 0) bad("ln: K = " + std::to_string(a.K) + " must be a multiple of 64");
    if (pn && a.K / 16 > 128) bad("pn: n_stat = K / 16 = " + std::to_string(a.K / 16) + " exceeds 128 statistics tiles per row");
    if (pn && !a.stat_in) bad("pn: null stat_in");
    const bool uses_ld = a.epilogue == DEPI_BIAS_T || a.epilogue == DEPI_BIAS_RESID || a.epilogue == DEPI_LOGITS;
    if (uses_ld && a.ld_out < a.N) bad("ld_out = " + std::to_string(a.ld_out) + " is below N = " + std::to_string(a.N));
    if (a.epilogue == DEPI_BIAS_GELU_T && a.N % 32 != 0) bad("BIAS_GELU_T writes activation tiles: N = " + std::to_string(a.N) + " must be a multiple of 32");
    const bool rows_epi = a.epilogue == DEPI_QKV || a.epilogue == DEPI_LOGITS;
    if (rows_epi && (a.n_new < 1 || a.M % a.n_new != 0)) bad("M = " + std::to_string(a.M) + " must be a multiple of n_new = " + std::to_string(a.n_new) + " >= 1");
    const int windows = rows_epi ? a.M / a.n_new : 0;
    if (a.epilogue == DEPI_QKV) {
      if (!a.k_cache || !a.v_cache || !a.n_past) bad("QKV: null k_cache, v_cache or n_past");
      if (a.n_head < 1 || a.n_ctx < 1 || a.d_model != 64 * a.n_head || a.N != 3 * a.d_model) bad("QKV: d_model == 64 * n_head, N == 3 * d_model, n_ctx >= 1");
      for (int b = 0; b < windows; ++b)
        if (a.n_past[b] < 0 || a.n_past[b] > a.n_ctx)
          bad("n_past[" + std::to_string(b) + "] = " + std::to_string(a.n_past[b]) + " is outside 0 .. n_ctx = " + std::to_string(a.n_ctx));
    }
    const int64_t tiles = (int64_t)((a.N + 15) / 16) * ((a.M + 31) / 32);
    if (a.ksplit > 1) {
      if (a.epilogue != DEPI_BIAS_RESID) bad("split-K exists for the RESID epilogue only");
      if (a.ksplit > a.K / 32) bad("ksplit = " + std::to_string(a.ksplit) + " exceeds the K / 32 = " + std::to_string(a.K / 32) + " k-blocks");
      if (!a.slab || !a.ticket) bad("split-K: null slab or ticket");
      if (a.slab_bytes < tiles * a.ksplit * 2048 || a.slab_bytes > INT32_MAX)
        bad("split-K: slab_bytes = " + std::to_string(a.slab_bytes) + ", needed " + std::to_string(tiles * a.ksplit * 2048) + " (tiles * ksplit * 2 KiB, below 2 GiB)");
    }
    if ((a.x16_out == nullptr) != (a.stat_out == nullptr)) bad("x16_out and stat_out come together");
    if (a.stat_out) {
      if (a.epilogue != DEPI_BIAS_RESID || a.ksplit > 1) bad("stat_out: statistics come from the unsplit RESID epilogue");
      if (a.N % 32 != 0) bad("stat_out: N = " + std::to_string(a.N) + " must be a multiple of 32");
    }

    hipStream_t s = (hipStream_t)stream;
    const int64_t n_pad = ((int64_t)a.N + 15) / 16 * 16;
    DevBuf wf, bf, wt, ws, past, lnr;
    // private copies, prepared as the loader prepares a decoder linear (model.hip): fold, round + tile, row sums
    wf.alloc((size_t)a.N * a.K * 4);
    HIP_CHECK(hipMemcpyAsync(wf.p, a.w, (size_t)a.N * a.K * 4, hipMemcpyDeviceToDevice, s));
    const bool own_bias = a.bias != nullptr || a.gamma != nullptr;
    if (own_bias) {
      bf.alloc((size_t)a.N * 4);
      if (a.bias) HIP_CHECK(hipMemcpyAsync(bf.p, a.bias, (size_t)a.N * 4, hipMemcpyDeviceToDevice, s));
      else HIP_CHECK(hipMemsetAsync(bf.p, 0, (size_t)a.N * 4, s));
    }
    if (a.gamma) launch_fold_ln(wf.as<float>(), bf.as<float>(), a.gamma, a.beta, a.N, a.K, s);
    wt.alloc((size_t)n_pad * a.K * 2);
    if (pn) ws.alloc((size_t)a.N * 4);
    if (ln) lnr.alloc(((size_t)a.M + 15) / 16 * 16 * a.K * 2);      // the LayerNorm launch of the all-rows forms
    if (a.epilogue == DEPI_QKV) dbg_upload(past, a.n_past, (size_t)windows);
    int shape = -1;
    Dispatch::run(a.dtype, [&](auto* tag) {
      using TT = std::remove_pointer_t<decltype(tag)>;
      launch_repack_tiled<TT>(wf.as<float>(), wt.p, a.N, n_pad, a.K, s);
      if (pn) launch_tiled_rowsum<TT>(wt.p, ws.as<float>(), a.N, a.K, s);
      DecGemmParams p{};
      p.x = a.x; p.ln = ln ? 1 : 0; p.ln_rows = lnr.p; p.w = wt.p; p.bias = own_bias ? bf.as<float>() : nullptr; p.out = a.out;
      p.M = a.M; p.N = a.N; p.K = a.K; p.n_new = rows_epi ? a.n_new : 1;
      p.ld_out = a.epilogue == DEPI_QKV ? a.d_model : a.ld_out; p.cu_budget = a.cu_budget;
      if (a.epilogue == DEPI_QKV) {
        p.k_cache = a.k_cache; p.v_cache = a.v_cache; p.n_past = past.as<int32_t>();
        p.d_model = a.d_model; p.n_head = a.n_head; p.n_ctx = a.n_ctx;
      }
      if (a.ksplit > 1) { p.ksplit = a.ksplit; p.slab = a.slab; p.slab_bytes = (int32_t)a.slab_bytes; p.ticket = a.ticket; }
      if (pn) { p.pn = 1; p.n_stat = a.K / 16; p.stat_in = a.stat_in; p.wsum = ws.as<float>(); }
      if (a.stat_out) { p.x16_out = a.x16_out; p.stat_out = a.stat_out; }
      if (a.epilogue == DEPI_LOGITS && out_all) { p.out_all = out_all; p.ld_all = ld_all; }
      shape = launch_dec_gemm<TT>(p, a.epilogue, s);
    });
    HIP_CHECK(hipStreamSynchronize(s));
    if (a.shape_out) *a.shape_out = shape;
  }
}
extern "C" {
int ohw_dbg_dec_gemm(const ohw_dbg_dec_gemm_io* io, void* stream) {
  return guard([&] { dbg_dec_gemm_run(io, nullptr, 0, stream); });
}

int ohw_dbg_logits_rows(const ohw_dbg_logits_rows_io* io, void* stream) {
  return guard([&] {
    if (!io) throw Error(OHW_E_INVALID_ARG, "dbg_logits_rows: null io");
    if (io->g.epilogue != DEPI_LOGITS) throw Error(OHW_E_INVALID_ARG, "dbg_logits_rows: the epilogue must be LOGITS");
    if (io->out_all && io->ld_all < io->g.N)
      throw Error(OHW_E_INVALID_ARG, "dbg_logits_rows: ld_all = " + std::to_string(io->ld_all) + " is below N = " + std::to_string(io->g.N));
    dbg_dec_gemm_run(&io->g, io->out_all, io->ld_all, stream);
  });
}

int ohw_dbg_token_score(ohw_state* st, const float* logits, int batch, int64_t ld, int n_vocab, int eot, const int32_t* targets,
                        const int32_t* n_all, int row0, int n_prompt, int cap, int guard_n, ohw_token_score* out) {
  return guard([&] {
    if (!st || !logits || !targets || !n_all || !out) throw Error(OHW_E_INVALID_ARG, "dbg_token_score: null argument");
    if (batch < 1 || batch > 4096 || n_vocab < 1 || n_vocab > (1 << 20) || ld < n_vocab || ld > (1 << 21) || ld % 4 != 0 || eot < 0 || row0 < 0 ||
        row0 > (1 << 20) || n_prompt < 1 || n_prompt > (1 << 20) || cap < 1 || cap > (1 << 16) || guard_n < 0 || guard_n > 4096)
      throw Error(OHW_E_INVALID_ARG, "dbg_token_score: bad shape");
    const int rows = batch * 8;
    for (int m = 0; m < rows; ++m)
      if (targets[m] < 0 || targets[m] >= n_vocab) throw Error(OHW_E_INVALID_ARG, "dbg_token_score: row " + std::to_string(m) + " has a target outside 0 .. n_vocab - 1");
    HIP_CHECK(hipSetDevice(st->ctx->device));
    hipStream_t s = st->stream;
    HIP_CHECK(hipStreamSynchronize(s));
    const size_t n_out = (size_t)batch * cap + 2 * (size_t)guard_n;
    DevBuf d_logits, d_tgt, d_cnt, d_out;
    d_logits.alloc(((size_t)rows + 2) * ld * 4);
    d_tgt.alloc((size_t)rows * 4); d_cnt.alloc((size_t)batch * 4); d_out.alloc(n_out * sizeof(ohw_token_score));
    const std::vector<float> nan_row((size_t)ld, std::numeric_limits<float>::quiet_NaN());
    ohw_token_score sent;
    sent.logit = sent.lse_text = sent.lse_all = sent.top_logit = OHW_DBG_SENTINEL_F32; sent.top_id = OHW_DBG_SENTINEL_I32;
    const std::vector<ohw_token_score> sent_out(n_out, sent);
    HIP_CHECK(hipMemcpyAsync(d_logits.p, nan_row.data(), (size_t)ld * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_logits.as<float>() + ld, logits, (size_t)rows * ld * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_logits.as<float>() + ((size_t)rows + 1) * ld, nan_row.data(), (size_t)ld * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_tgt.p, targets, (size_t)rows * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_cnt.p, n_all, (size_t)batch * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_out.p, sent_out.data(), n_out * sizeof(ohw_token_score), hipMemcpyHostToDevice, s));
    TokenScoreParams tp{};
    tp.logits = d_logits.as<float>() + ld; tp.ld = ld; tp.targets = d_tgt.as<int32_t>(); tp.n_all = d_cnt.as<int32_t>();
    tp.row0 = row0; tp.n_prompt = n_prompt; tp.n_vocab = n_vocab; tp.eot = eot; tp.batch = batch; tp.cap = cap;
    tp.out = d_out.as<ohw_token_score>() + guard_n;
    launch_token_score(tp, s);
    HIP_CHECK(hipMemcpyAsync(out, d_out.p, n_out * sizeof(ohw_token_score), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  });
}

int ohw_dbg_embed(int dtype, const float* emb, int n_vocab, const float* pos, int n_pos, const int32_t* tok_host,
                  const int32_t* n_past_host, float* x, void* x16, float* stat, int M, int n_new, int d, void* stream) {
  return guard([&] {
    dbg_check_dtype(dtype, "dbg_embed");
    if (!emb || !pos || !tok_host || !n_past_host || !x || n_vocab < 1 || n_pos < 1 || M < 1 || n_new < 1 || d < 32)
      throw Error(OHW_E_INVALID_ARG, "dbg_embed: null buffer, or n_vocab, n_pos, M or n_new below 1, or d below 32");
    if (d % 32 != 0 || d > (1 << 16) || n_vocab > (1 << 20)) throw Error(OHW_E_INVALID_ARG, "dbg_embed: d must be a multiple of 32 (at most 2^16), n_vocab at most 2^20");
    if (M % n_new != 0) throw Error(OHW_E_INVALID_ARG, "dbg_embed: M must be a multiple of n_new");
    for (int m = 0; m < M; ++m)
      if (tok_host[m] < 0 || tok_host[m] >= n_vocab)
        throw Error(OHW_E_INVALID_ARG, "dbg_embed: tok[" + std::to_string(m) + "] = " + std::to_string(tok_host[m]) + " is outside the " + std::to_string(n_vocab) + " rows of the table");
    for (int b = 0; b < M / n_new; ++b)
      if (n_past_host[b] < 0 || (int64_t)n_past_host[b] + n_new > n_pos)
        throw Error(OHW_E_INVALID_ARG, "dbg_embed: n_past[" + std::to_string(b) + "] = " + std::to_string(n_past_host[b]) + " with n_new = " + std::to_string(n_new) +
                                           " is outside the " + std::to_string(n_pos) + " positions");
    hipStream_t s = (hipStream_t)stream;
    const int64_t v_pad = ((int64_t)n_vocab + 15) / 16 * 16;
    DevBuf et, tok, past;
    et.alloc((size_t)v_pad * d * 2);
    dbg_upload(tok, tok_host, (size_t)M);
    dbg_upload(past, n_past_host, (size_t)(M / n_new));
    Dispatch::run(dtype, [&](auto* tag) {
      using TT = std::remove_pointer_t<decltype(tag)>;
      launch_repack_tiled<TT>(emb, et.p, n_vocab, v_pad, d, s);
      launch_embed<TT>(et.p, pos, tok.as<int32_t>(), past.as<int32_t>(), x, x16, stat, M, n_new, d, s);
    });
    HIP_CHECK(hipStreamSynchronize(s));
  });
}

int ohw_dbg_layernorm(int dtype, const float* x, const float* gamma, const float* beta, void* y, int64_t rows, int d, int tiled,
                      void* stream) {
  return guard([&] {
    dbg_check_dtype(dtype, "dbg_layernorm");
    if (!x || !gamma || !beta || !y || rows < 1 || rows > (1 << 24)) throw Error(OHW_E_INVALID_ARG, "dbg_layernorm: null buffer, or rows outside 1 .. 2^24");
    if (d < 4 || d % 4 != 0 || d > 2048) throw Error(OHW_E_INVALID_ARG, "dbg_layernorm: d must be a multiple of 4 in 4 .. 2048");
    if (tiled && d % 32 != 0) throw Error(OHW_E_INVALID_ARG, "dbg_layernorm: the tiled output needs d % 32 == 0");
    Dispatch::run(dtype, [&](auto* tag) {
      using TT = std::remove_pointer_t<decltype(tag)>;
      launch_layernorm<TT>(x, gamma, beta, y, rows, d, (hipStream_t)stream, tiled != 0);
    });
    HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  });
}

static_assert(OHW_EG_KERNEL_AUTO == 0 && OHW_EG_KERNEL_K128 == 1 && OHW_EG_KERNEL_SMALL == 2 && OHW_EG_KERNEL_K256 == 3, "ohw.h names the encoder GEMM kernels");

int ohw_dbg_enc_gemm(const ohw_dbg_enc_gemm_io* io, void* stream) {
  return guard([&] {
    if (!io) throw Error(OHW_E_INVALID_ARG, "dbg_enc_gemm: null io");
    const ohw_dbg_enc_gemm_io& a = *io;
    auto bad = [](const std::string& why) { throw Error(OHW_E_INVALID_ARG, "dbg_enc_gemm: " + why); };
    auto str = [](int64_t v) { return std::to_string(v); };
    auto aligned16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
    dbg_check_dtype(a.dtype, "dbg_enc_gemm");
    if (a.epilogue < EPI_BIAS_T || a.epilogue > EPI_CROSSKV_T) bad("epilogue must be 0 .. 5");
    if (a.kernel < OHW_EG_KERNEL_AUTO || a.kernel > OHW_EG_KERNEL_K256) bad("kernel must be 0 (auto), 1 (128x128), 2 (64x64) or 3 (256x256)");
    if (!a.a || !a.w || !a.out) bad("null a, w or out");
    const int64_t lim = (int64_t)1 << 20;
    if (a.M < 1 || a.N < 64 || a.K < 64 || a.M > lim || a.N > lim || a.K > lim) bad("M >= 1, N >= 64 and K >= 64 (each at most 2^20)");
    if (a.K % 64 != 0) bad("K = " + str(a.K) + " must be a multiple of 64");
    const int64_t n_mult = a.kernel == OHW_EG_KERNEL_K256 ? 256 : a.kernel == OHW_EG_KERNEL_SMALL ? 64 : 128;
    if (a.N % n_mult != 0) bad("N = " + str(a.N) + " must be a multiple of " + str(n_mult) + " for this kernel");
    if (a.rows_per_batch < 1 || a.rows_per_batch > lim) bad("rows_per_batch must be 1 .. 2^20");
    if (a.lda < 0 || a.a_batch_stride < 0 || a.lda > ((int64_t)1 << 30) || a.a_batch_stride > ((int64_t)1 << 30)) bad("lda and a_batch_stride must lie in 0 .. 2^30");
    if (a.lda % 8 != 0 || a.a_batch_stride % 8 != 0 || !aligned16(a.a)) bad("lda and a_batch_stride must be multiples of 8 elements and a 16-byte aligned");
    if (a.a_elems < 0 || a.out_elems < 0) bad("negative a_elems or out_elems");
    // the last element any row reads: window nb - 1, its last row, K columns
    const int64_t nb = (a.M + a.rows_per_batch - 1) / a.rows_per_batch, rows = std::min(a.M, a.rows_per_batch);
    const int64_t a_need = (nb - 1) * a.a_batch_stride + (rows - 1) * a.lda + a.K;
    if (a_need > a.a_elems) bad("the rows of A end at element " + str(a_need) + ", past a_elems = " + str(a.a_elems));
    if (a.bias && !aligned16(a.bias)) bad("bias must be 16-byte aligned");
    if (!aligned16(a.out)) bad("out must be 16-byte aligned");
    if (a.c_row_map && a.epilogue != EPI_CROSSKV_T) bad("a row map goes with the cross-K/V epilogue only");
    if (a.conv_cin < 0) bad("conv_cin must not be negative");
    if (a.conv_cin > 0 && (a.K % 3 != 0 || a.conv_cin > a.K / 3)) bad("conv weights: K must be 3 * c_pad with conv_cin <= c_pad");
    if (a.epilogue == EPI_CROSSKV_T) {
      if (a.n_head < 1 || a.n_head > 1024 || a.d_model != 64 * a.n_head || a.N % a.d_model != 0) bad("cross-K/V: d_model == 64 * n_head and N a multiple of d_model");
      if (a.t_len < 1 || a.t_len > lim || a.batch < 1 || a.batch > lim || a.batch_offset < 0 || a.batch_offset >= a.batch)
        bad("cross-K/V: t_len and batch in 1 .. 2^20, 0 <= batch_offset < batch");
      const double need = (double)(a.N / a.d_model) * a.batch * a.n_head * a.t_len * 64.0;   // exact below 2^53; out_elems is far below
      if (need > (double)a.out_elems) bad("cross-K/V: the slabs hold more than out_elems = " + str(a.out_elems) + " elements");
      if (a.c_row_map) {
        const int64_t top = (int64_t)(a.batch - a.batch_offset) * a.t_len;
        for (int64_t m = 0; m < a.M; ++m)
          if (a.c_row_map[m] < 0 || a.c_row_map[m] >= top)
            bad("c_row_map[" + str(m) + "] = " + str(a.c_row_map[m]) + " is outside 0 .. " + str(top - 1));
      } else {
        if (rows > a.t_len) bad("cross-K/V: " + str(rows) + " rows per window exceed t_len = " + str(a.t_len));
        if (a.batch_offset + nb > a.batch) bad("cross-K/V: windows " + str(a.batch_offset) + " .. " + str(a.batch_offset + nb - 1) + " exceed batch = " + str(a.batch));
      }
    } else {
      const bool f32_out = a.epilogue == EPI_BIAS_RESID_F32 || a.epilogue == EPI_GELU_POS_F32 || a.epilogue == EPI_F32;
      const int64_t el16 = f32_out ? 4 : 8;   // elements in 16 bytes
      if (a.ldc < a.N || a.ldc > ((int64_t)1 << 30) || a.c_batch_stride < 0 || a.c_batch_stride > ((int64_t)1 << 30)) bad("N <= ldc <= 2^30 and 0 <= c_batch_stride <= 2^30");
      if (a.ldc % el16 != 0 || a.c_batch_stride % el16 != 0) bad("ldc and c_batch_stride must be multiples of 16 bytes");
      if (nb > 1 && a.c_batch_stride < (rows - 1) * a.ldc + a.N) bad("c_batch_stride = " + str(a.c_batch_stride) + ": the output windows overlap");
      const int64_t need = (nb - 1) * a.c_batch_stride + (rows - 1) * a.ldc + a.N;
      if (need > a.out_elems) bad("the output rows end at element " + str(need) + ", past out_elems = " + str(a.out_elems));
      if (a.epilogue == EPI_GELU_POS_F32 && (!a.pos || !aligned16(a.pos))) bad("GELU_POS_F32 needs pos, 16-byte aligned");
    }

    hipStream_t s = (hipStream_t)stream;
    DevBuf wt, map;
    wt.alloc((size_t)a.N * a.K * 2);
    if (a.c_row_map) dbg_upload(map, a.c_row_map, (size_t)a.M);
    Dispatch::run(a.dtype, [&](auto* tag) {
      using TT = std::remove_pointer_t<decltype(tag)>;
      // the weights as the loader prepares them (model.hip): a linear's rows rounded, a convolution's taps repacked
      if (a.conv_cin > 0) launch_repack_conv<TT>(a.w, wt.p, a.N, a.conv_cin, a.K / 3, s);
      else launch_convert_rows<TT>(a.w, wt.p, a.N, a.K, a.K, s);
      GemmParams g{};
      g.A = a.a; g.W = wt.p; g.bias = a.bias; g.out = a.out; g.pos = a.epilogue == EPI_GELU_POS_F32 ? a.pos : nullptr;
      g.M = a.M; g.N = a.N; g.K = a.K;
      g.lda = a.lda; g.a_batch_stride = a.a_batch_stride; g.rows_per_batch = a.rows_per_batch;
      g.ldc = a.ldc; g.c_batch_stride = a.c_batch_stride;
      if (a.epilogue == EPI_CROSSKV_T) {
        g.d_model = a.d_model; g.n_head = a.n_head; g.t_len = a.t_len; g.batch = a.batch; g.batch_offset = a.batch_offset;
        g.c_row_map = a.c_row_map ? map.as<int32_t>() : nullptr;
      }
      switch (a.kernel) {
        case OHW_EG_KERNEL_K128: launch_gemm128<TT>(g, a.epilogue, s); break;
        case OHW_EG_KERNEL_SMALL: launch_gemm_small<TT>(g, a.epilogue, s); break;
        case OHW_EG_KERNEL_K256: launch_gemm256<TT>(g, a.epilogue, s); break;
        default: launch_gemm<TT>(g, a.epilogue, s); break;
      }
    });
    HIP_CHECK(hipStreamSynchronize(s));
  });
}

}  // extern "C"
