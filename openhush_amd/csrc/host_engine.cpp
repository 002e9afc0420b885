// host_engine.cpp — the host side above the C ABI: a C++ mirror of the reference's WhisperEngine
// (reference src/engine/whisper.rs:110-387) written in C++ because the build image has no Rust
// toolchain.  Same method set, argument meaning and error behaviour:
//   ohw_engine_new         <- WhisperEngine::new          (:129-179)
//   ohw_engine_transcribe  <- WhisperEngine::transcribe   (:204-310)
//   ohw_engine_benchmark   <- WhisperEngine::benchmark    (:334-387)
//   ohw_validate_audio     <- validation::validate_audio  (src/engine/validation.rs:46-118)
//   ohw_lang_id_to_code    <- lang_id_to_code             (:627-731)
// The host owns 30 s windowing and (optionally) the token sampler, as BASELINE.json asks; the
// arithmetic is in the HIP library.  There is no CPU fallback: use_gpu = false is an error.
#include <sys/stat.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <memory>
#include <random>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "common.hpp"
#include "model.hpp"

namespace ohw {
extern thread_local std::string g_last_error;
const float* state_bias_host(const ohw_state* st);
void state_share_recording(ohw_state* dst, ohw_state* src);
void state_drop_recording(ohw_state* st);
void state_set_graph_max_batch(ohw_state* st, int max_batch);
}
extern "C" const ohw_ctx* ohw_state_ctx(const ohw_state* st);
using namespace ohw;

namespace {
const char* const kLangs[99] = {
    "en", "zh", "de", "es", "ru", "ko", "fr", "ja", "pt", "tr", "pl", "ca", "nl", "ar", "sv", "it", "id", "hi", "fi", "vi",
    "he", "uk", "el", "ms", "cs", "ro", "da", "hu", "ta", "no", "th", "ur", "hr", "bg", "lt", "la", "mi", "ml", "cy", "sk",
    "te", "fa", "lv", "bn", "sr", "az", "sl", "kn", "et", "mk", "br", "eu", "is", "hy", "ne", "mn", "bs", "kk", "sq", "sw",
    "gl", "mr", "pa", "si", "km", "sn", "yo", "so", "af", "oc", "ka", "be", "tg", "sd", "gu", "am", "yi", "lo", "uz", "fo",
    "ht", "ps", "tk", "nn", "mt", "sa", "lb", "my", "bo", "tl", "mg", "as", "tt", "haw", "ln", "ha", "ba", "jw", "su"};

template <typename F>
int guard(F&& f) {
  ApiScope api;
  try {
    f();
    return OHW_OK;
  } catch (const Error& e) {
    g_last_error = e.what();
    return e.code;
  } catch (const std::exception& e) {
    g_last_error = e.what();
    return OHW_E_TRANSCRIBE;
  } catch (...) {
    g_last_error = "unknown error";
    return OHW_E_TRANSCRIBE;
  }
}
}  // namespace

#include "host_engine.hpp"

// ---- the seek loops of many recordings, one window of each live one per round (include/ohw.h, ohw_seek_sched_*) -----------
// Host only.  The engine's long-form batch runs on this object and holds no second copy of the bookkeeping.
struct ohw_seek_sched {
  int max_batch = 1;
  std::vector<int32_t> seek, seek_end;     // per recording, 10 ms frames
  std::vector<int32_t> waiting;            // live recordings that hold no slot yet: longest first, equal lengths in submission order
  size_t next_waiting = 0;
  std::vector<int32_t> slot_rec;           // per slot: the recording it holds, -1 = free
  std::vector<int32_t> slot_fresh;         // per slot: taken since the last round
  std::vector<int32_t> round_rec;          // the last round: recording of entry b
  bool live(int r) const { return seek_end[(size_t)r] >= 100 && seek[(size_t)r] + 100 < seek_end[(size_t)r]; }
};

namespace {
// ---- whisper.cpp's per-window bookkeeping (whisper_full_with_state as recalled) ---------
struct SeqEval {
  int n_sampled = 0;     // tokens up to and including the one that ended the pass
  int result_len = 0;    // whisper.cpp result_len: up to and including the last timestamp token (> token_beg)
  int n_keep = 0;        // tokens that reach the text
  int seek_delta = 3000; // 10 ms frames the window advances by
  bool failed = false, completed = false;
  float avg_logprob = -INFINITY, entropy = 0.f;
};

// frames of 10 ms whisper.cpp attributes to n samples: mel.n_len_org = 1 + (n + 200 - 400) / 160
int mel_frames(int64_t n) { return (int)(1 + (n + 200 - 400) / 160); }

// One sampled sequence, judged after the fact (greedy decoding is causal: cutting at the first exit the walk finds equals
// having stopped there).  tok[0..n): the sampled tokens, the end-of-text token last when it was sampled.
//   exits      end-of-text; a timestamp that leaves less than 1 s of audio (seek + seek_delta + 100 >= seek_end);
//              failure when timestamps go back, when end-of-text arrives with no timestamp and audio left, or when the
//              loop reaches n_max without a timestamp past the middle of the window (the repetition-loop guard)
//   score      average log-probability and token-frequency entropy of the last 32 of the first result_len tokens
//   kept       fixed 30 s cuts: everything before the exit (each window is decoded once); seek loop: result_len tokens
//              (what follows the last timestamp is decoded again by the next window)
SeqEval evaluate_sequence(const ohw_special_tokens& tk, const int32_t* tok, const float* plog, int n, int seek, int seek_end, int n_max,
                          bool no_timestamps, int window_mode) {
  SeqEval r;
  bool has_ts = false;
  int stop = n;
  for (int i = 0; i < n; ++i) {
    const int t = tok[i];
    if (t > tk.timestamp_begin) {
      const int nd = 2 * (t - tk.timestamp_begin);
      if (has_ts && r.seek_delta > nd && r.result_len < i) { r.failed = true; stop = i + 1; break; }
      r.seek_delta = nd; r.result_len = i + 1; has_ts = true;
    }
    const bool audio_end = seek + r.seek_delta + 100 >= seek_end;
    if (t == tk.eot || (has_ts && audio_end)) {
      if (r.result_len == 0 && !no_timestamps) {
        if (audio_end) r.result_len = i + 1;
        else { r.failed = true; stop = i + 1; break; }
      }
      if (no_timestamps) { r.result_len = i + 1; r.seek_delta = 3000; }
      r.completed = true; stop = i + 1;
      break;
    }
    if (i == n_max - 1 && (r.result_len == 0 || r.seek_delta < 1500)) { r.failed = true; stop = i + 1; break; }
  }
  r.n_sampled = stop;
  if (r.result_len > 0) {
    double sum = 0.0;
    for (int i = 0; i < r.result_len; ++i) sum += plog[i];
    r.avg_logprob = (float)(sum / r.result_len);
    const int n32 = std::min(32, r.result_len), i0 = r.result_len - n32;
    double ent = 0.0;
    for (int i = i0; i < r.result_len; ++i) {
      bool first = true;
      int cnt = 0;
      for (int j = i0; j < r.result_len; ++j) if (tok[j] == tok[i]) { if (j < i) first = false; ++cnt; }
      if (first) { const double pr = (double)cnt / n32; ent -= pr * std::log(pr); }
    }
    r.entropy = (float)ent;
  }
  int keep = r.failed ? stop : (window_mode == OHW_WINDOW_SEEK ? r.result_len : stop);
  while (keep > 0 && tok[keep - 1] == tk.eot) --keep;
  r.n_keep = keep;
  return r;
}

bool needs_fallback(const SeqEval& r, const ohw_decode_policy& q, float no_speech_prob, bool is_last) {
  if (is_last) return false;
  const bool failed = r.failed || r.result_len == 0 || r.entropy < q.entropy_thold;
  return failed || (r.avg_logprob < q.logprob_thold && no_speech_prob < q.no_speech_thold);
}

struct WindowRun {
  std::vector<int32_t> tok;   // sampled tokens of the kept pass (end-of-text last when sampled)
  std::vector<float> plog;
  float nosp = 0.f, temp = 0.f;
  SeqEval ev;
  bool pending = false, t0_failed = false;
  std::vector<int32_t> al_idx;   // word timestamps: start index of every kept text token, then the end of the last (empty: not aligned)
};

std::vector<float> ladder(const ohw_decode_policy& q) {
  std::vector<float> t;
  if (q.temperature_inc > 0.0f)
    for (float x = q.temperature_inc; x < 1.0f + 1e-6f && t.size() < 16; x += q.temperature_inc) t.push_back(x);
  return t;
}
}  // namespace

namespace ohw {

ohw_engine* engine_wrap_ctx(ohw_ctx* ctx, const std::string& language, bool translate, int max_batch, int device) {
  std::unique_ptr<ohw_engine> e(new ohw_engine());
  e->language = language;
  e->translate = translate;
  e->max_batch = std::max(1, max_batch);
  e->device = device;
  if (const char* ev = getenv("OHW_ENGINE_ENC_CUS")) e->enc_cus = std::max(0, atoi(ev));
  if (const char* ev = getenv("OHW_ENGINE_LANES")) e->lanes = std::min(16, std::max(1, atoi(ev)));
  if (const char* ev = getenv("OHW_ENGINE_MERGE")) e->merge = std::min(8, std::max(1, atoi(ev)));
  if (e->max_batch * e->merge > 256) e->merge = std::max(1, 256 / e->max_batch);     // a state holds at most 256 windows
  if (const char* ev = getenv("OHW_ENGINE_SCHEDULE")) {
    const std::string v = ev;
    e->schedule = v == "sequential" ? OHW_SCHEDULE_SEQUENTIAL : v == "pipeline" ? OHW_SCHEDULE_PIPELINE : OHW_SCHEDULE_LANES;
  }
  const int rc = ohw_state_create(ctx, e->max_batch, &e->state);
  if (rc != OHW_OK) throw Error(rc == OHW_E_OOM ? rc : OHW_E_LOAD_FAILED, "Failed to create state: " + g_last_error);
  e->ctx = ctx;
  e->packed_encoder = ohw_state_packed_encoder(e->state) == 1;     // OHW_ENC_PACKED
  return e.release();
}

void trim_spans(std::vector<ohw_span_time>& v, size_t lead, size_t new_len) {
  for (ohw_span_time& s : v) {
    size_t o0 = std::max(s.text_off, lead) - lead, o1 = std::max(s.text_off + s.text_len, lead) - lead;
    o0 = std::min(o0, new_len); o1 = std::min(o1, new_len);
    s.text_off = o0; s.text_len = o1 - o0;
  }
}

bool engine_detects(const ohw_engine* e) { return e->detect_language && e->language == "auto" && e->ctx->hp.n_vocab >= 51865; }

int32_t engine_detect_first_window(ohw_engine* e, const float* samples, int64_t n, float* prob) {
  auto check = [&](int rc) { if (rc != OHW_OK) throw Error(OHW_E_TRANSCRIBE, "Language detection failed: " + g_last_error); };
  if (prob) *prob = 0.f;
  if (mel_frames(n) < 100) return 0;          // less than 1 s: the call yields nothing, whatever the language
  const int full_ctx = e->ctx->hp.n_audio_ctx;
  const int call_ctx = e->audio_ctx > 0 ? e->audio_ctx : (e->audio_ctx < 0 && n <= CHUNK_SAMPLES) ? std::min<int>(ohw_audio_ctx_for(n), full_ctx) : 0;
  ohw_state* st = e->state;
  check(ohw_state_set_stream(st, nullptr));
  check(ohw_state_set_audio_ctx(st, call_ctx));
  if (e->window_mode == OHW_WINDOW_FIXED) {
    const int32_t n0 = (int32_t)std::min<int64_t>(CHUNK_SAMPLES, n);
    check(ohw_mel(st, samples, n0, &n0, 1, 0, OHW_MEL_ZERO_TAIL, nullptr));
  } else {
    const int32_t seek0 = 0;
    check(ohw_recording_set(st, samples, n, 0, nullptr));
    check(ohw_mel_seek(st, &seek0, 1, nullptr));
  }
  check(ohw_encode(st, 1));
  struct Clear { ohw_state* st; ~Clear() { (void)ohw_state_set_window_lang(st, nullptr, 0); } } clear{st};
  int32_t id = OHW_LANG_DETECT;
  check(ohw_state_set_window_lang(st, &id, 1));
  check(ohw_state_detect_window_lang(st, 1));
  std::vector<float> probs((size_t)e->ctx->tok.n_langs);
  check(ohw_state_window_lang(st, 1, &id, probs.data()));
  if (id < 0 || id >= e->ctx->tok.n_langs) throw Error(OHW_E_TRANSCRIBE, "Language detection failed: no id");
  if (prob) *prob = probs[(size_t)id];
  return id;
}

void engine_transcribe_core(ohw_engine* e, const float* samples, int64_t n, std::string* text_out, int64_t win_first, int64_t win_step,
                            const ohw_audio_span* recs, int n_recs, const int32_t* rec_langs, bool long_batch) {
  std::string own_text;
  std::string& text = text_out ? *text_out : own_text;
  if (win_first < 0 || win_step < 1) throw Error(OHW_E_INVALID_ARG, "transcribe: window dealing must be first >= 0, step >= 1");
    ohw_sample_params sp;
    ohw_default_sample_params(e->ctx, &sp);
    // reference :246-248: "auto" skips set_language and whisper.cpp keeps its default "en"
    sp.lang_id = e->language == "auto" ? 0 : ohw_lang_code_to_id(e->language.c_str());
    // reference :251-257 passes !translate to whisper-rs on the claim that the binding is inverted;
    // the resulting behaviour the reference documents is: config translate=true -> translate task
    sp.translate = e->translate ? 1 : 0;
    if (e->force_len > 0) { sp.force_len = std::min(e->force_len, sp.n_max); sp.n_max = sp.force_len; }      // bench: fixed decode length
    const ohw_special_tokens& tk = e->ctx->tok;
    if (sp.lang_id >= tk.n_langs) throw Error(OHW_E_TRANSCRIBE, "language is not supported by this model");
    // ohw_engine_set_detect_language: one detection per call, on the first window (or the id the pool detected); every window
    // of every schedule then runs at that id, exactly as an engine created with its code
    e->last_lang_id = sp.lang_id;
    e->last_lang_prob = 1.f;
    if (!recs && engine_detects(e)) {
      if (e->given_lang >= 0) { e->last_lang_id = e->given_lang; e->last_lang_prob = e->given_prob; }
      else e->last_lang_id = engine_detect_first_window(e, samples, n, &e->last_lang_prob);
      sp.lang_id = e->last_lang_id;
    }
    // ohw_engine_transcribe_batch with languages per recording: the ids of the batch being decoded (empty: sp.lang_id for all)
    std::vector<int32_t> batch_lang;

    e->last_tokens.clear();
    e->last_quality.clear();
    e->last_trace.clear();
    e->last_token_times.clear(); e->last_words.clear(); e->last_segments.clear(); e->last_marks.clear(); e->last_contexts.clear();
    const int max_tok = e->ctx->hp.n_text_ctx;
    const int V = e->ctx->hp.n_vocab;
    const int n_max = sp.n_max;
    const ohw_decode_policy& pol = e->policy;
    const std::vector<float> temps = ladder(pol);
    // ohw_engine_set_beam_size: the T = 0 pass is a beam search of K rows per window, so a decode batch holds max_batch / K
    // windows; everything that cuts batches below takes WB.  Beam calls run one batch after the other on the engine's own state
    const int beam_K = e->beam_size;
    const int WB = beam_K > 0 ? e->max_batch / beam_K : e->max_batch;
    if (WB < 1) throw Error(OHW_E_INVALID_ARG, "transcribe: beam size exceeds max_batch");
    int32_t prompt[8];
    int n_prompt = 0;
    prompt[n_prompt++] = tk.sot;
    if (V >= 51865) { prompt[n_prompt++] = tk.sot + 1 + sp.lang_id; prompt[n_prompt++] = sp.translate ? tk.translate : tk.transcribe; }
    if (sp.no_timestamps) prompt[n_prompt++] = tk.no_timestamps;
    auto check = [&](int rc) { if (rc != OHW_OK) throw Error(OHW_E_TRANSCRIBE, "Transcription failed: " + g_last_error); };   // reference :266-268
    // per-decode scratch: one per lane when several batches decode side by side
    struct Scratch {
      std::vector<int32_t> toks, ntok, eot, trace;
      std::vector<float> lps, nsp, logits;
      std::vector<WindowRun> runs;
      Scratch(int B, int max_tok) : toks((size_t)B * max_tok), ntok((size_t)B), eot((size_t)B), lps((size_t)B * (max_tok + 1)), nsp((size_t)B) {}
    };
    auto trace = [&](Scratch& sc, int64_t window, float temp, const std::vector<int32_t>& t) {
      sc.trace.push_back((int32_t)window); sc.trace.push_back((int32_t)std::lround(temp * 1000.f)); sc.trace.push_back((int32_t)t.size());
      sc.trace.insert(sc.trace.end(), t.begin(), t.end());
    };

    // the initial prompt (ohw_engine_set_initial_prompt) as the context of every window of the batch; with none set and none
    // ever set, nothing is called.  The ladder clears the table before its first pass with T >= 0.5 (whisper.cpp's rule, as
    // recalled), so every batch sets it again here
    // carried context (ohw_engine_set_carry_context; the seek loops only): one history per recording of the call, seeded with the
    // initial prompt and moved on by ohw_carry_step_host after every window; `next` is what the recording's next window decodes
    // behind at T = 0.  round_ctx[b]: the context of decode-batch entry b of the round being decoded
    const bool carrying = e->carry_max != 0 && e->window_mode == OHW_WINDOW_SEEK;
    struct Carry { std::vector<int32_t> hist, next; int n_hist = 0; };
    std::vector<const std::vector<int32_t>*> round_ctx;
    const std::vector<int32_t>* emit_ctx = nullptr;         // what emit() records as the window's context (null: the initial prompt)
    auto carry_step = [&](Carry& c, const int32_t* kept, int n_kept, float temp) {
      std::vector<int32_t> out((size_t)std::max(1, max_tok / 2));
      int n_out = 0;
      const int rc = ohw_carry_step_host(c.hist.data(), &c.n_hist, max_tok, kept, n_kept, temp, e->carry_max, out.data(), &n_out);
      if (rc != OHW_OK) throw Error(rc, "carry_context: " + g_last_error);
      c.next.assign(out.begin(), out.begin() + n_out);
    };
    auto carry_init = [&](Carry& c) {
      c.hist.assign((size_t)std::max(1, max_tok / 2), 0);
      c.n_hist = (int)std::min(e->prompt.size(), c.hist.size());
      std::copy(e->prompt.end() - c.n_hist, e->prompt.end(), c.hist.begin());
      carry_step(c, nullptr, 0, 0.f);
    };
    auto apply_prompt = [&](ohw_state* st, int B) {
      if (carrying) {
        // a slot whose history is empty gets count 0; a round in which every history is empty runs with no table at all
        size_t np = 0;
        for (int b = 0; b < B; ++b) np = std::max(np, round_ctx[(size_t)b]->size());
        if (np == 0) {
          if (e->prompt_used) check(ohw_state_set_window_prompt(st, nullptr, 0, nullptr, 0));
          return;
        }
        std::vector<int32_t> tab((size_t)B * np, 0), cnt((size_t)B, 0);
        for (int b = 0; b < B; ++b) {
          cnt[(size_t)b] = (int32_t)round_ctx[(size_t)b]->size();
          std::copy(round_ctx[(size_t)b]->begin(), round_ctx[(size_t)b]->end(), tab.begin() + (long)((size_t)b * np));
        }
        e->prompt_used = true;
        check(ohw_state_set_window_prompt(st, tab.data(), (int)np, cnt.data(), B));
        return;
      }
      if (e->prompt.empty()) {
        if (e->prompt_used) check(ohw_state_set_window_prompt(st, nullptr, 0, nullptr, 0));
        return;
      }
      const int np = (int)e->prompt.size();
      std::vector<int32_t> tab((size_t)B * np), cnt((size_t)B, np);
      for (int b = 0; b < B; ++b) std::memcpy(&tab[(size_t)b * np], e->prompt.data(), (size_t)np * 4);
      check(ohw_state_set_window_prompt(st, tab.data(), np, cnt.data(), B));
    };
    // T = 0: the device-resident greedy loop for B windows; then whisper.cpp's bookkeeping per window
    auto greedy_t0 = [&](Scratch& sc, ohw_state* st, int B, const int* seek, const int* seek_end, int64_t w0) {
      apply_prompt(st, B);
      std::vector<int32_t>&toks = sc.toks, &ntok = sc.ntok, &eot = sc.eot;
      std::vector<float>&lps = sc.lps, &nsp = sc.nsp;
      std::vector<WindowRun>& runs = sc.runs;
      ohw_greedy_result gr{};
      gr.tokens = toks.data(); gr.n_tokens = ntok.data(); gr.token_logprobs = lps.data(); gr.ended_by_eot = eot.data(); gr.no_speech_prob = nsp.data();
      check(ohw_greedy_ex(st, &sp, B, max_tok, &gr));
      runs.assign((size_t)B, WindowRun());
      for (int b = 0; b < B; ++b) {
        WindowRun& r = runs[(size_t)b];
        const int nt = ntok[(size_t)b] + (eot[(size_t)b] ? 1 : 0);
        r.tok.assign(&toks[(size_t)b * max_tok], &toks[(size_t)b * max_tok] + ntok[(size_t)b]);
        if (eot[(size_t)b]) r.tok.push_back(tk.eot);
        r.plog.assign(&lps[(size_t)b * (max_tok + 1)], &lps[(size_t)b * (max_tok + 1)] + nt);
        r.nosp = nsp[(size_t)b];
        r.ev = evaluate_sequence(tk, r.tok.data(), r.plog.data(), nt, seek[b], seek_end[b], n_max, sp.no_timestamps != 0, e->window_mode);
        r.t0_failed = needs_fallback(r.ev, pol, r.nosp, false);
        r.pending = needs_fallback(r.ev, pol, r.nosp, temps.empty());
        trace(sc, w0 + b, 0.f, r.tok);
      }
    };
    // T = 0 under ohw_engine_set_beam_size: ohw_beam_search_ex in greedy_t0's place, filling the same WindowRun.  The winner (with
    // end-of-text when it came from the finished pool) is judged by evaluate_sequence and cut at n_sampled, as device_pass cuts a
    // sampled pass: beam search is not causal, so whisper.cpp's loop exits are applied to the winner after the search (a
    // definition), not to every decoder during it.  From there on it is the greedy pass: needs_fallback,
    // t0_failed, the no-speech rule, n_keep, segments, alignment.
    // The ladder that may follow is unchanged and safe after a search: it decodes rows 0 .. B-1 from position 0 (prefill,
    // prompt, steps), reads a row's self K/V only below the position it has itself written in that pass, without a kv_slot
    // table, and reads cross K/V by WINDOW index, which the search never moves - nothing it relies on is left in beam layout
    // (row w * K); its entries re-initialise n_past, the token history and the done flags themselves
    auto beam_t0 = [&](Scratch& sc, ohw_state* st, int B, const int* seek, const int* seek_end, int64_t w0) {
      apply_prompt(st, B);
      ohw_beam_result_ex br{};
      br.tokens = sc.toks.data(); br.n_tokens = sc.ntok.data(); br.token_logprobs = sc.lps.data(); br.ended_by_eot = sc.eot.data();
      br.no_speech_prob = sc.nsp.data();
      check(ohw_beam_search_ex(st, &sp, B, beam_K, max_tok, &br));
      sc.runs.assign((size_t)B, WindowRun());
      for (int b = 0; b < B; ++b) {
        WindowRun& r = sc.runs[(size_t)b];
        const int nt = sc.ntok[(size_t)b] + (sc.eot[(size_t)b] ? 1 : 0);
        r.tok.assign(&sc.toks[(size_t)b * max_tok], &sc.toks[(size_t)b * max_tok] + sc.ntok[(size_t)b]);
        if (sc.eot[(size_t)b]) r.tok.push_back(tk.eot);
        r.plog.assign(&sc.lps[(size_t)b * (max_tok + 1)], &sc.lps[(size_t)b * (max_tok + 1)] + nt);
        r.nosp = sc.nsp[(size_t)b];
        const SeqEval ev = evaluate_sequence(tk, r.tok.data(), r.plog.data(), nt, seek[b], seek_end[b], n_max, sp.no_timestamps != 0, e->window_mode);
        r.tok.resize((size_t)ev.n_sampled);
        r.plog.resize((size_t)ev.n_sampled);
        r.ev = evaluate_sequence(tk, r.tok.data(), r.plog.data(), (int)r.tok.size(), seek[b], seek_end[b], n_max, sp.no_timestamps != 0, e->window_mode);
        r.t0_failed = needs_fallback(r.ev, pol, r.nosp, false);
        r.pending = needs_fallback(r.ev, pol, r.nosp, temps.empty());
        trace(sc, w0 + b, 0.f, r.tok);
      }
    };
    auto pass_t0 = [&](Scratch& sc, ohw_state* st, int B, const int* seek, const int* seek_end, int64_t w0) {
      if (beam_K > 0) beam_t0(sc, st, B, seek, seek_end, w0);
      else greedy_t0(sc, st, B, seek, seek_end, w0);
    };
    // the temperature ladder for the windows of a batch whose pass failed the acceptance test, drawn from std::mt19937 through
    // std::discrete_distribution as whisper.cpp's decoders do, on the pending windows' resident cross K/V.  By default the
    // HOST samples: the device runs the decoder steps of the pending windows only and their logits cross PCIe every step.
    // e->fallback_device: the device samples too (ohw_sample_pass: the greedy loop's replayed {step, sampler} with the
    // temperature sampler), from the host generators' pre-drawn doubles; the host then cuts each pass at whisper.cpp's loop
    // exits (evaluate_sequence) and advances each generator by the draws it kept, where the host ladder would leave it
    auto device_pass = [&](Scratch& sc, ohw_state* st, int B, const int* seek, const int* seek_end, const std::vector<int32_t>& active, float T,
                           const std::vector<ohw_rng*>& rngs, std::vector<WindowRun>& pass) {
      std::vector<double> u((size_t)B * max_tok, 0.0);
      const int n_draw = std::min(n_max, max_tok);
      for (int b = 0; b < B; ++b)
        if (active[(size_t)b] && ohw_rng_uniforms(rngs[(size_t)b], n_draw, &u[(size_t)b * max_tok]) != OHW_OK) throw Error(OHW_E_TRANSCRIBE, "Transcription failed: generator");
      ohw_greedy_result gr{};
      gr.tokens = sc.toks.data(); gr.n_tokens = sc.ntok.data(); gr.token_logprobs = sc.lps.data(); gr.ended_by_eot = sc.eot.data(); gr.no_speech_prob = sc.nsp.data();
      check(ohw_sample_pass(st, &sp, B, max_tok, T, active.data(), u.data(), &gr));
      for (int b = 0; b < B; ++b) {
        if (!active[(size_t)b]) continue;
        WindowRun& r = pass[(size_t)b];
        const int nt = sc.ntok[(size_t)b] + (sc.eot[(size_t)b] ? 1 : 0);
        r.tok.assign(&sc.toks[(size_t)b * max_tok], &sc.toks[(size_t)b * max_tok] + sc.ntok[(size_t)b]);
        if (sc.eot[(size_t)b]) r.tok.push_back(tk.eot);
        r.plog.assign(&sc.lps[(size_t)b * (max_tok + 1)], &sc.lps[(size_t)b * (max_tok + 1)] + nt);
        r.nosp = sc.nsp[(size_t)b];
        const SeqEval ev = evaluate_sequence(tk, r.tok.data(), r.plog.data(), nt, seek[b], seek_end[b], n_max, sp.no_timestamps != 0, e->window_mode);
        r.tok.resize((size_t)ev.n_sampled);
        r.plog.resize((size_t)ev.n_sampled);
        if (ohw_rng_discard_draws(rngs[(size_t)b], ev.n_sampled) != OHW_OK) throw Error(OHW_E_TRANSCRIBE, "Transcription failed: generator");
      }
    };
    auto run_ladder = [&](Scratch& sc, ohw_state* st, int B, const int* seek, const int* seek_end, int64_t w0, const std::vector<ohw_rng*>& rngs) {
      std::vector<float>& logits = sc.logits;
      std::vector<WindowRun>& runs = sc.runs;
      for (size_t ti = 0; ti < temps.size(); ++ti) {
        std::vector<int32_t> active((size_t)B, 0);
        bool any = false;
        for (int b = 0; b < B; ++b) if (runs[(size_t)b].pending) { active[(size_t)b] = 1; any = true; }
        if (!any) break;
        const float T = temps[ti];
        const bool is_last = ti + 1 == temps.size();
        std::vector<WindowRun> pass((size_t)B);
        // passes with T < 0.5 decode behind the context; from the first pass with T >= 0.5 on the table is gone
        if (T >= 0.5f && (carrying || !e->prompt.empty())) check(ohw_state_set_window_prompt(st, nullptr, 0, nullptr, 0));
        if (e->fallback_device) {
          device_pass(sc, st, B, seek, seek_end, active, T, rngs, pass);
        } else {
          logits.resize((size_t)B * V);
          std::vector<int32_t> ptoks((size_t)B * n_prompt), past((size_t)B, 0), feed((size_t)B, tk.eot), npast((size_t)B, n_prompt), live = active;
          for (int b = 0; b < B; ++b) {
            std::memcpy(&ptoks[(size_t)b * n_prompt], prompt, (size_t)n_prompt * 4);
            if (!batch_lang.empty() && V >= 51865) ptoks[(size_t)b * n_prompt + 1] = tk.sot + 1 + batch_lang[(size_t)b];   // the table's ids, read back once per batch
          }
          // under a context table: the prefill for the pending windows, then the prompt at the context's length
          check(ohw_state_prefill(st, B, active.data()));
          for (int b = 0; b < B; ++b) {
            past[(size_t)b] = std::max(0, ohw_state_window_prompt_len(st, b));
            npast[(size_t)b] += past[(size_t)b];
          }
          check(ohw_decode_active(st, ptoks.data(), n_prompt, past.data(), B, active.data(), logits.data()));
          for (int i = 0; i < n_max; ++i) {
            bool any_live = false;
            for (int b = 0; b < B; ++b) {
              if (!live[(size_t)b]) continue;
              WindowRun& r = pass[(size_t)b];
              float lp = 0.f;
              if (const float* bias = state_bias_host(st))          // the state's logit bias: the device sampler adds it itself
                for (int i2 = 0; i2 < V; ++i2) logits[(size_t)b * V + i2] += bias[i2];
              const int32_t t = ohw_sample_host(e->ctx, &sp, &logits[(size_t)b * V], r.tok.data(), (int)r.tok.size(), T, rngs[(size_t)b], &lp, &r.nosp);
              if (t < 0) throw Error(OHW_E_TRANSCRIBE, "Transcription failed: host sampler");
              r.tok.push_back(t); r.plog.push_back(lp);
              const SeqEval ev = evaluate_sequence(tk, r.tok.data(), r.plog.data(), (int)r.tok.size(), seek[b], seek_end[b], n_max,
                                                   sp.no_timestamps != 0, e->window_mode);
              if (t == tk.eot || ev.completed || ev.failed || (int)r.tok.size() >= n_max || npast[(size_t)b] + 1 >= max_tok) live[(size_t)b] = 0;
              else { feed[(size_t)b] = t; any_live = true; }
            }
            if (!any_live) break;
            check(ohw_decode_active(st, feed.data(), 1, npast.data(), B, live.data(), logits.data()));
            for (int b = 0; b < B; ++b) if (live[(size_t)b]) ++npast[(size_t)b];
          }
        }
        for (int b = 0; b < B; ++b) {
          if (!active[(size_t)b]) continue;
          WindowRun& r = pass[(size_t)b];
          r.temp = T;
          r.ev = evaluate_sequence(tk, r.tok.data(), r.plog.data(), (int)r.tok.size(), seek[b], seek_end[b], n_max, sp.no_timestamps != 0, e->window_mode);
          r.t0_failed = runs[(size_t)b].t0_failed;
          r.pending = needs_fallback(r.ev, pol, r.nosp, is_last);
          trace(sc, w0 + b, T, r.tok);
          runs[(size_t)b] = std::move(r);
        }
      }
    };
    // word timestamps: the kept pass of every window of a batch is aligned on the state that decoded it, while its cross K/V
    // is resident (before that state's next encode); windows with no kept text token are skipped.  frames: 10 ms frames of audio
    auto kept_tokens = [&](const WindowRun& r) {
      const bool no_speech = r.nosp > pol.no_speech_thold && r.ev.avg_logprob < pol.logprob_thold;
      return no_speech ? 0 : r.ev.n_keep;
    };
    auto align_runs = [&](Scratch& sc, ohw_state* st, int B, const int* frames) {
      if (e->wt_heads.empty()) return;
      const int half = e->ctx->hp.n_text_ctx / 2;
      std::vector<int32_t> atok((size_t)B * half, 0), nt((size_t)B, 0), nf((size_t)B, 0), out((size_t)B * (half + 1), 0);
      bool any = false;
      for (int b = 0; b < B; ++b) {
        WindowRun& r = sc.runs[(size_t)b];
        r.al_idx.clear();
        const int keep = kept_tokens(r);
        int k = 0;
        for (int i = 0; i < keep && k < half; ++i)
          if (r.tok[(size_t)i] < tk.eot) atok[(size_t)b * half + k++] = r.tok[(size_t)i];
        nt[(size_t)b] = k;
        nf[(size_t)b] = std::max(0, frames[b]);
        any = any || k > 0;
      }
      if (!any) return;
      check(ohw_state_set_align_heads(st, e->wt_heads.data(), (int)e->wt_heads.size()));
      check(ohw_state_align(st, &sp, atok.data(), half, nt.data(), nf.data(), B, out.data()));
      for (int b = 0; b < B; ++b)
        if (nt[(size_t)b] > 0) sc.runs[(size_t)b].al_idx.assign(&out[(size_t)b * (half + 1)], &out[(size_t)b * (half + 1)] + nt[(size_t)b] + 1);
    };
    // t_off: the window's offset in the recording, t_end: the earlier of the window's end and the recording's end (seconds)
    auto emit = [&](const WindowRun& r, double t_off, double t_end) {
      // whisper.cpp (>= 1.7.3 as recalled): a window whose no-speech probability is high AND whose text is unlikely is dropped
      const bool no_speech = r.nosp > pol.no_speech_thold && r.ev.avg_logprob < pol.logprob_thold;
      const int keep = no_speech ? 0 : r.ev.n_keep;
      ohw_engine::WindowMark mark;
      mark.text0 = text.size();
      const size_t tt0 = e->last_token_times.size(), wd0 = e->last_words.size(), sg0 = e->last_segments.size();
      std::vector<size_t> byte_off((size_t)keep + 1, text.size());       // text offset in front of every kept token
      std::vector<int32_t> tlen;                                         // byte length of every kept TEXT token
      std::vector<int> tpos;                                             //   and its position among the kept tokens
      const size_t win_text0 = text.size();
      for (int i = 0; i < keep; ++i) {
        byte_off[(size_t)i] = text.size();
        e->last_tokens.push_back(r.tok[(size_t)i]);
        if (r.tok[(size_t)i] < tk.eot) {                                    // segment text = text tokens only (:271-279)
          const char* sp_ = nullptr;
          const int len = ohw_token_text(e->ctx, r.tok[(size_t)i], &sp_);
          text.append(sp_, (size_t)len);
          tlen.push_back(len); tpos.push_back(i);
        }
      }
      byte_off[(size_t)keep] = text.size();
      if (keep > 0) {
        // segments (always): the text between consecutive timestamp tokens
        std::vector<ohw_token_span> spans((size_t)keep);
        const int ns_ = ohw_segments_host(r.tok.data(), keep, &tk, (float)t_off, (float)t_end, spans.data(), keep);
        for (int s = 0; s < ns_; ++s) {
          const size_t o0 = byte_off[(size_t)spans[(size_t)s].first], o1 = byte_off[(size_t)spans[(size_t)s].end];
          e->last_segments.push_back(ohw_span_time{o0, o1 - o0, spans[(size_t)s].t0, spans[(size_t)s].t1});
        }
      }
      if (!r.al_idx.empty() && r.al_idx.size() == tlen.size() + 1) {
        // token times, and words by the host rule (include/ohw.h)
        const int32_t window = (int32_t)e->last_quality.size();
        const size_t first_tt = e->last_token_times.size();
        for (size_t k = 0; k < tlen.size(); ++k)
          e->last_token_times.push_back(ohw_token_time{r.tok[(size_t)tpos[k]], window, (float)t_off + (float)r.al_idx[k] * 0.02f,
                                                       (float)t_off + (float)r.al_idx[k + 1] * 0.02f});
        std::vector<int32_t> starts(tlen.size(), 0);
        (void)ohw_word_starts_host(text.data() + win_text0, tlen.data(), (int)tlen.size(), starts.data());
        for (size_t k = 0; k < tlen.size(); ++k) {
          const ohw_token_time& tt = e->last_token_times[first_tt + k];
          const size_t o0 = byte_off[(size_t)tpos[k]];
          if (starts[k] || e->last_words.size() == wd0) e->last_words.push_back(ohw_span_time{o0, 0, tt.t0, tt.t1});
          ohw_span_time& w = e->last_words.back();
          w.text_len = o0 + (size_t)tlen[k] - w.text_off;
          w.t1 = tt.t1;
        }
      }
      mark.n_token_times = (int32_t)(e->last_token_times.size() - tt0);
      mark.n_words = (int32_t)(e->last_words.size() - wd0);
      mark.n_segments = (int32_t)(e->last_segments.size() - sg0);
      e->last_marks.push_back(mark);
      e->last_contexts.push_back(emit_ctx ? *emit_ctx : e->prompt);
      ohw_window_quality q{};
      q.n_tokens = keep; q.avg_logprob = r.ev.avg_logprob; q.entropy = r.ev.entropy; q.would_fallback = r.t0_failed ? 1 : 0;
      q.temperature = r.temp; q.no_speech_prob = r.nosp; q.no_speech = no_speech ? 1 : 0; q.seek_delta = r.ev.seek_delta;
      q.result_len = r.ev.result_len; q.failed = r.ev.failed ? 1 : 0;
      e->last_quality.push_back(q);
    };
    struct Rngs {   // whisper.cpp seeds every decoder's generator with 0 once per whisper_full call
      std::vector<ohw_rng*> v;
      ~Rngs() { for (ohw_rng* r : v) ohw_rng_free(r); }
      void reset(size_t nr) { for (ohw_rng* r : v) ohw_rng_free(r); v.clear(); for (size_t i = 0; i < nr; ++i) v.push_back(ohw_rng_new(0)); }
    } rngs;

    // a batch records its passes in the order it ran them (every window's T = 0 pass, then the ladder's rungs); the trace lists
    // them window by window, each window's passes in order, so it reads the same however the windows were batched
    auto flush_trace = [&](Scratch& sc) {
      std::vector<std::pair<int32_t, size_t>> recs;            // (window, offset of the record)
      for (size_t i = 0; i + 3 <= sc.trace.size(); i += 3 + (size_t)sc.trace[i + 2]) recs.emplace_back(sc.trace[i], i);
      std::stable_sort(recs.begin(), recs.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
      for (const auto& r : recs) e->last_trace.insert(e->last_trace.end(), sc.trace.begin() + (long)r.second, sc.trace.begin() + (long)(r.second + 3 + (size_t)sc.trace[r.second + 2]));
      sc.trace.clear();
    };
    // the audio context of this call (ohw_engine_set_audio_ctx), on every state it may run on: auto = the context that covers a
    // recording of at most one window, the full context for anything longer
    const int full_ctx = e->ctx->hp.n_audio_ctx;
    const int call_ctx = e->audio_ctx > 0 ? e->audio_ctx : (e->audio_ctx < 0 && n <= CHUNK_SAMPLES) ? std::min<int>(ohw_audio_ctx_for(n), full_ctx) : 0;
    auto apply_ctx = [&] {
      check(ohw_state_set_audio_ctx(e->state, call_ctx));
      for (ohw_state* st : e->states) check(ohw_state_set_audio_ctx(st, call_ctx));
      for (ohw_state* st : e->lane_states) check(ohw_state_set_audio_ctx(st, call_ctx));
    };
    // a fixed context never drops audio silently: a window that holds samples past it fails the call
    auto check_window_fits = [&](int64_t window, int64_t win_samples) {
      if (call_ctx > 0 && win_samples > (int64_t)call_ctx * 320)
        throw Error(OHW_E_INVALID_ARG, "audio_ctx " + std::to_string(call_ctx) + " covers " + std::to_string((int64_t)call_ctx * 320) + " samples, window " +
                                           std::to_string(window) + " holds " + std::to_string(win_samples));
    };
    // the decode of one batch on whatever stream the state is set to; fills sc.runs (and sc.trace); re-entrant per Scratch
    auto decode_windows = [&](Scratch& sc, ohw_state* st, int64_t w0, int B, const int32_t* nsb) {
      std::vector<int> zero((size_t)B, 0), ends((size_t)B);
      for (int b = 0; b < B; ++b) ends[(size_t)b] = mel_frames(nsb[b]);
      pass_t0(sc, st, B, zero.data(), ends.data(), w0);
      for (int b = 0; b < B; ++b) if (ends[(size_t)b] <= 100) { sc.runs[(size_t)b] = WindowRun(); sc.runs[(size_t)b].ev.result_len = 0; }
      bool any = false;
      for (int b = 0; b < B; ++b) any = any || sc.runs[(size_t)b].pending;
      if (any) {
        Rngs lr;
        lr.reset((size_t)B);
        run_ladder(sc, st, B, zero.data(), ends.data(), w0, lr.v);
      }
      align_runs(sc, st, B, ends.data());
    };

    if (recs && long_batch) {
      // ---- ohw_engine_transcribe_long_batch: the seek loop of every recording, one window of each live recording per round,
      // on the engine's own state.  Each recording is one whisper_full call: its own generator across all its windows, its own
      // frame count as the end of the audio, the full audio context (what the single loop runs anything longer than a window
      // at).  The caller has set e->window_mode to OHW_WINDOW_SEEK for the call.
      e->batch_records.assign((size_t)n_recs, ohw_engine::BatchRecord());
      const int MB = WB;
      std::vector<int64_t> lens((size_t)n_recs);
      for (int i = 0; i < n_recs; ++i) lens[(size_t)i] = recs[i].n;
      ohw_seek_sched* sched_raw = nullptr;
      const int src = ohw_seek_sched_new(lens.data(), n_recs, MB, &sched_raw);
      if (src != OHW_OK) throw Error(src, g_last_error);
      struct SchedFree { ohw_seek_sched* s; ~SchedFree() { ohw_seek_sched_free(s); } } sched_free{sched_raw};
      struct Restore {
        ohw_engine* e;
        explicit Restore(ohw_engine* e_) : e(e_) { (void)ohw_state_set_batch_invariant(e->state, 1); }
        ~Restore() { (void)ohw_state_set_batch_invariant(e->state, 0); (void)ohw_state_set_window_lang(e->state, nullptr, 0); }
      } restore_state(e);
      const bool per_rec = V >= 51865 && (rec_langs != nullptr || engine_detects(e));
      if (rec_langs)
        for (int i = 0; i < n_recs; ++i)
          if (rec_langs[i] != OHW_LANG_DETECT && (rec_langs[i] < 0 || rec_langs[i] >= tk.n_langs))
            throw Error(OHW_E_INVALID_ARG, "transcribe_long_batch: recording " + std::to_string(i) + " asks for language id " + std::to_string(rec_langs[i]));
      check(ohw_state_set_stream(e->state, nullptr));
      check(ohw_state_set_audio_ctx(e->state, 0));
      check(ohw_state_set_window_ctx(e->state, nullptr, 0));
      // what emit() appends to, per recording: swapped into the engine's last_* records around every emit
      struct Acc {
        std::string text; std::vector<int32_t> tokens; std::vector<ohw_window_quality> quality;
        std::vector<ohw_token_time> token_times; std::vector<ohw_span_time> words, segments; std::vector<ohw_engine::WindowMark> marks;
        std::vector<std::vector<int32_t>> contexts;
      };
      std::vector<Acc> acc((size_t)n_recs);
      auto swap_acc = [&](Acc& a) {
        text.swap(a.text); e->last_tokens.swap(a.tokens); e->last_quality.swap(a.quality); e->last_token_times.swap(a.token_times);
        e->last_words.swap(a.words); e->last_segments.swap(a.segments); e->last_marks.swap(a.marks);
        e->last_contexts.swap(a.contexts);
      };
      // a recording's language: the caller's id, or OHW_LANG_DETECT until its first window has been detected (with no table: -1)
      std::vector<int32_t> rec_lang((size_t)n_recs, -1);
      if (per_rec) for (int i = 0; i < n_recs; ++i) rec_lang[(size_t)i] = rec_langs ? rec_langs[i] : OHW_LANG_DETECT;
      rngs.reset((size_t)n_recs);
      // a history follows its recording, not the slot: a refilled slot starts from its new recording's own history
      std::vector<Carry> carry((size_t)(carrying ? n_recs : 0));
      for (Carry& c : carry) carry_init(c);
      round_ctx.assign((size_t)MB, nullptr);
      Scratch sc(MB, max_tok);
      std::vector<int32_t> r_rec((size_t)MB), r_slot((size_t)MB), r_seek((size_t)MB), r_fresh((size_t)MB);
      std::vector<int> seeks((size_t)MB), ends((size_t)MB), frames((size_t)MB);
      std::vector<ohw_rng*> round_rngs((size_t)MB);
      for (;;) {
        const int B = ohw_seek_sched_round(sched_raw, r_rec.data(), r_slot.data(), r_seek.data(), r_fresh.data());
        if (B < 0) throw Error(OHW_E_TRANSCRIBE, "Transcription failed: " + g_last_error);
        if (B == 0) break;
        for (int b = 0; b < B; ++b) {
          const int i = r_rec[(size_t)b];
          if (r_fresh[(size_t)b]) check(ohw_recording_set_slot(e->state, r_slot[(size_t)b], recs[i].samples, recs[i].n, 0, nullptr));
          seeks[(size_t)b] = r_seek[(size_t)b];
          ends[(size_t)b] = mel_frames(recs[i].n);
          frames[(size_t)b] = std::min(CHUNK_FRAMES, ends[(size_t)b] - seeks[(size_t)b]);
          round_rngs[(size_t)b] = rngs.v[(size_t)i];
          if (carrying) round_ctx[(size_t)b] = &carry[(size_t)i].next;
        }
        check(ohw_mel_seek_slots(e->state, r_slot.data(), r_seek.data(), B, nullptr));
        check(ohw_encode(e->state, B));
        if (per_rec) {
          batch_lang.assign((size_t)B, OHW_LANG_DETECT);
          bool any_detect = false;
          for (int b = 0; b < B; ++b) {
            batch_lang[(size_t)b] = rec_lang[(size_t)r_rec[(size_t)b]];
            any_detect = any_detect || batch_lang[(size_t)b] == OHW_LANG_DETECT;
          }
          check(ohw_state_set_window_lang(e->state, batch_lang.data(), B));
          if (any_detect) {
            // whisper.cpp detects once per whisper_full call, on the first window: read back once, kept for the later windows
            check(ohw_state_detect_window_lang(e->state, B));
            check(ohw_state_window_lang(e->state, B, batch_lang.data(), nullptr));
            for (int b = 0; b < B; ++b) rec_lang[(size_t)r_rec[(size_t)b]] = batch_lang[(size_t)b];
          }
        }
        pass_t0(sc, e->state, B, seeks.data(), ends.data(), 0);
        run_ladder(sc, e->state, B, seeks.data(), ends.data(), 0, round_rngs);
        align_runs(sc, e->state, B, frames.data());
        sc.trace.clear();
        for (int b = 0; b < B; ++b) {
          const int i = r_rec[(size_t)b];
          const WindowRun& r = sc.runs[(size_t)b];
          swap_acc(acc[(size_t)i]);
          emit_ctx = carrying ? round_ctx[(size_t)b] : nullptr;
          emit(r, seeks[(size_t)b] * 0.01, std::min(seeks[(size_t)b] * 0.01 + 30.0, (double)recs[i].n / 16000.0));
          swap_acc(acc[(size_t)i]);
          if (carrying) carry_step(carry[(size_t)i], r.tok.data(), kept_tokens(r), r.temp);
            check(ohw_seek_sched_advance(sched_raw, b, r.ev.seek_delta));
        }
      }
      if (carrying) check(ohw_state_set_window_prompt(e->state, nullptr, 0, nullptr, 0));
      for (int i = 0; i < n_recs; ++i) {
        Acc& a = acc[(size_t)i];
        ohw_engine::BatchRecord& r = e->batch_records[(size_t)i];
        const size_t b0 = a.text.find_first_not_of(" \t\r\n"), b1 = a.text.find_last_not_of(" \t\r\n");
        r.text = b0 == std::string::npos ? std::string() : a.text.substr(b0, b1 - b0 + 1);
        trim_spans(a.words, b0 == std::string::npos ? 0 : b0, r.text.size());
        trim_spans(a.segments, b0 == std::string::npos ? 0 : b0, r.text.size());
        r.tokens = std::move(a.tokens); r.qualities = std::move(a.quality); r.contexts = std::move(a.contexts);
        r.token_times = std::move(a.token_times); r.words = std::move(a.words); r.segments = std::move(a.segments);
        if (!r.qualities.empty()) r.quality = r.qualities[0];
        // a recording that never ran a window (under 1 s) was never detected: id 0, as the single loop reports it
        r.lang_id = !per_rec ? -1 : rec_lang[(size_t)i] == OHW_LANG_DETECT ? 0 : rec_lang[(size_t)i];
      }
      text.clear(); e->last_tokens.clear(); e->last_quality.clear();
      e->last_token_times.clear(); e->last_words.clear(); e->last_segments.clear(); e->last_marks.clear(); e->last_contexts.clear();
      return;
    }
    if (recs) {
      // ---- ohw_engine_transcribe_batch: every recording one window of its own; longest first, max_batch at a time, one batch
      // after the other on the engine's own state.  Under the auto setting a batch's envelope is its largest context and every
      // window runs at its own (ohw_state_set_window_ctx) - unless all of them equal the envelope, which is the uniform path
      e->batch_records.assign((size_t)n_recs, ohw_engine::BatchRecord());
      std::vector<int64_t> lens((size_t)n_recs);
      for (int i = 0; i < n_recs; ++i) lens[(size_t)i] = recs[i].n;
      const int MB = WB, n_b = (n_recs + MB - 1) / MB;
      std::vector<int32_t> order((size_t)n_recs), rctx((size_t)n_recs), env((size_t)n_b);
      const int prc = ohw_batch_plan(lens.data(), n_recs, MB, e->audio_ctx, order.data(), rctx.data(), env.data());
      if (prc != OHW_OK) throw Error(prc, g_last_error);
      struct Restore {
        ohw_engine* e;
        explicit Restore(ohw_engine* e_) : e(e_) { (void)ohw_state_set_batch_invariant(e->state, 1); }
        ~Restore() {
          (void)ohw_state_set_window_ctx(e->state, nullptr, 0); (void)ohw_state_set_batch_invariant(e->state, 0);
          (void)ohw_state_set_window_lang(e->state, nullptr, 0);
        }
      } restore_state(e);
      Scratch sc(MB, max_tok);
      std::vector<float> stage;
      std::vector<int32_t> ns((size_t)MB), wl((size_t)MB);
      // a language per recording: the caller's ids, or a detection per recording when the engine detects; an English-only model
      // has no language token and stays as it is
      const bool per_rec = V >= 51865 && (rec_langs != nullptr || engine_detects(e));
      if (rec_langs)
        for (int i = 0; i < n_recs; ++i)
          if (rec_langs[i] != OHW_LANG_DETECT && (rec_langs[i] < 0 || rec_langs[i] >= tk.n_langs))
            throw Error(OHW_E_INVALID_ARG, "transcribe_batch: recording " + std::to_string(i) + " asks for language id " + std::to_string(rec_langs[i]));
      for (int bi = 0; bi < n_b; ++bi) {
        const int B = std::min(MB, n_recs - bi * MB);
        const int32_t* ord = &order[(size_t)bi * MB];
        const int E = std::min<int>(env[(size_t)bi], full_ctx);
        bool ragged = false;
        for (int b = 0; b < B; ++b) {
          ns[(size_t)b] = (int32_t)recs[ord[b]].n;
          wl[(size_t)b] = std::min<int>(rctx[(size_t)ord[b]], full_ctx);
          ragged = ragged || wl[(size_t)b] != E;
        }
        const int64_t stride = ns[0];       // the longest of the batch
        stage.assign((size_t)(stride * B), 0.0f);
        for (int b = 0; b < B; ++b) std::memcpy(&stage[(size_t)(stride * b)], recs[ord[b]].samples, (size_t)ns[(size_t)b] * sizeof(float));
        check(ohw_state_set_audio_ctx(e->state, E));
        check(ohw_state_set_window_ctx(e->state, ragged ? wl.data() : nullptr, ragged ? B : 0));
        check(ohw_mel(e->state, stage.data(), stride, ns.data(), B, 0, OHW_MEL_ZERO_TAIL, nullptr));
        check(ohw_encode(e->state, B));
        if (per_rec) {
          batch_lang.assign((size_t)B, OHW_LANG_DETECT);
          bool any_detect = false;
          for (int b = 0; b < B; ++b) {
            if (rec_langs) batch_lang[(size_t)b] = rec_langs[ord[b]];
            any_detect = any_detect || batch_lang[(size_t)b] == OHW_LANG_DETECT;
          }
          check(ohw_state_set_window_lang(e->state, batch_lang.data(), B));
          if (any_detect) check(ohw_state_detect_window_lang(e->state, B));
          check(ohw_state_window_lang(e->state, B, batch_lang.data(), nullptr));      // the one read-back of the batch
        }
        decode_windows(sc, e->state, (int64_t)bi * MB, B, ns.data());
        sc.trace.clear();
        for (int b = 0; b < B; ++b) {
          text.clear(); e->last_tokens.clear(); e->last_quality.clear();
          e->last_token_times.clear(); e->last_words.clear(); e->last_segments.clear(); e->last_marks.clear(); e->last_contexts.clear();
          emit(sc.runs[(size_t)b], 0.0, (double)recs[ord[b]].n / 16000.0);
          ohw_engine::BatchRecord& r = e->batch_records[(size_t)ord[b]];
          const size_t b0 = text.find_first_not_of(" \t\r\n"), b1 = text.find_last_not_of(" \t\r\n");
          r.text = b0 == std::string::npos ? std::string() : text.substr(b0, b1 - b0 + 1);
          trim_spans(e->last_words, b0 == std::string::npos ? 0 : b0, r.text.size());
          trim_spans(e->last_segments, b0 == std::string::npos ? 0 : b0, r.text.size());
          r.token_times = e->last_token_times; r.words = e->last_words; r.segments = e->last_segments;
          r.tokens = e->last_tokens;
          r.quality = e->last_quality[0];
          r.lang_id = per_rec ? batch_lang[(size_t)b] : -1;
        }
      }
      text.clear(); e->last_tokens.clear(); e->last_quality.clear();
      e->last_token_times.clear(); e->last_words.clear(); e->last_segments.clear(); e->last_marks.clear(); e->last_contexts.clear();
      return;
    }
    if (e->window_mode == OHW_WINDOW_SEEK) {
      // whisper.cpp's seek loop as recalled: sequential windows, advanced by the last timestamp; one
      // generator for the whole call
      rngs.reset(1);
      Scratch sc(1, max_tok);
      Carry carry;
      if (carrying) { carry_init(carry); round_ctx.assign(1, &carry.next); emit_ctx = &carry.next; }
      const int seek_end = mel_frames(n);
      int seek = 0;
      int64_t w = 0;
      // whisper.cpp computes the log-mel spectrogram of the whole input once (the clamp uses its global maximum) and every
      // window reads 3000 frames of it at its seek offset
      if (seek_end >= 100) check(ohw_recording_set(e->state, samples, n, 0, nullptr));
      apply_ctx();
      while (seek_end >= 100 && seek + 100 < seek_end) {
        const int32_t seek32 = seek;
        check_window_fits(w, std::min<int64_t>(CHUNK_SAMPLES, n - (int64_t)seek * HOP));
        check(ohw_mel_seek(e->state, &seek32, 1, nullptr));      // 3000 frames of the recording-wide spectrogram
        check(ohw_encode(e->state, 1));
        pass_t0(sc, e->state, 1, &seek, &seek_end, w);
        run_ladder(sc, e->state, 1, &seek, &seek_end, w, rngs.v);
        const int win_frames = std::min(CHUNK_FRAMES, seek_end - seek);
        align_runs(sc, e->state, 1, &win_frames);
        flush_trace(sc);
        emit(sc.runs[0], seek * 0.01, std::min(seek * 0.01 + 30.0, (double)n / 16000.0));
        if (carrying) carry_step(carry, sc.runs[0].tok.data(), kept_tokens(sc.runs[0]), sc.runs[0].temp);
        seek += sc.runs[0].ev.seek_delta > 0 ? sc.runs[0].ev.seek_delta : 3000;
        ++w;
      }
      if (carrying && w > 0) check(ohw_state_set_window_prompt(e->state, nullptr, 0, nullptr, 0));
    } else {
      // host-side windowing: fixed 30 s cuts (BASELINE.json north_star).  Each cut is its own `full` call in
      // whisper.cpp terms: seek 0, its own frame count as the end of the audio, a fresh generator - and, like a call with
      // less than 1 s of audio (`seek + 100 >= seek_end` before the first window), a cut of at most 100 frames yields nothing
      // the pool deals the recording's windows round-robin: this engine takes windows win_first, win_first + win_step, ... of
      // the WHOLE recording it is handed (no copy, and - FIXED_RECORDING_MEL - the real neighbouring samples and the
      // recording-wide clamp maximum); k counts this engine's windows, rec_win(k) is the window of the recording
      const int64_t n_win_rec = (n + CHUNK_SAMPLES - 1) / CHUNK_SAMPLES;
      const int64_t n_win = n_win_rec > win_first ? (n_win_rec - win_first + win_step - 1) / win_step : 0;
      auto rec_win = [&](int64_t k) { return win_first + k * win_step; };
      for (int64_t k = 0; k < n_win; ++k) check_window_fits(rec_win(k), std::min<int64_t>(CHUNK_SAMPLES, n - rec_win(k) * CHUNK_SAMPLES));
      const int64_t n_batches = (n_win + WB - 1) / WB;
      auto batch_of = [&](int64_t bi) { return (int)std::min<int64_t>(WB, n_win - bi * WB); };
      // windows w0 .. w0 + B of the recording into st: each cut on its own (its own `full()` call), or cut from the spectrogram
      // of the whole recording (FIXED_RECORDING_MEL: st reads the recording e->state holds)
      const bool rec_mel = e->window_mode == OHW_WINDOW_FIXED_RECORDING_MEL;
      auto mel_windows = [&](ohw_state* st, int64_t w0, int B, const int32_t* nsv) {
        if (!rec_mel) { check(ohw_mel(st, samples + rec_win(w0) * CHUNK_SAMPLES, win_step * CHUNK_SAMPLES, nsv, B, 0, OHW_MEL_ZERO_TAIL, nullptr)); return; }
        std::vector<int32_t> seeks((size_t)B);
        for (int b = 0; b < B; ++b) seeks[(size_t)b] = (int32_t)(rec_win(w0 + b) * CHUNK_FRAMES);
        check(ohw_mel_seek(st, seeks.data(), B, nullptr));
      };
      if (rec_mel) check(ohw_recording_set(e->state, samples, n, 0, nullptr));
      auto fill_ns = [&](int64_t bi, std::vector<int32_t>& nsv) {
        const int64_t w0 = bi * WB;
        const int B = batch_of(bi);
        for (int b = 0; b < B; ++b) nsv[(size_t)b] = (int32_t)std::min<int64_t>(CHUNK_SAMPLES, n - rec_win(w0 + b) * CHUNK_SAMPLES);
      };
      auto front = [&](int64_t bi, ohw_state* st, void* stream, std::vector<int32_t>& nsv) {
        fill_ns(bi, nsv);
        check(ohw_state_set_stream(st, stream));
        mel_windows(st, bi * WB, batch_of(bi), nsv.data());
        check(ohw_encode(st, batch_of(bi)));
      };
      auto decode_batch = [&](Scratch& sc, ohw_state* st, int64_t bi, const int32_t* nsb) { decode_windows(sc, st, bi * WB, batch_of(bi), nsb); };
      auto collect = [&](Scratch& sc, int B, int64_t w0) {
        flush_trace(sc);
        for (int b = 0; b < B; ++b) {
          const double t_off = (double)rec_win(w0 + b) * 30.0;
          emit(sc.runs[(size_t)b], t_off, std::min(t_off + 30.0, (double)n / 16000.0));
        }
      };
      int schedule = n_batches > 1 ? e->schedule : OHW_SCHEDULE_SEQUENTIAL;
      if (beam_K > 0) schedule = OHW_SCHEDULE_SEQUENTIAL;      // no lanes for beams: the serial path on the engine's own state
      if (schedule == OHW_SCHEDULE_LANES && e->lanes < 2) schedule = OHW_SCHEDULE_SEQUENTIAL;
      if (schedule == OHW_SCHEDULE_PIPELINE && e->enc_cus <= 0) schedule = OHW_SCHEDULE_SEQUENTIAL;
      // ---- resources of the overlapped schedules, made when a long input first needs them: more states, CU-masked streams ----
      if (schedule != OHW_SCHEDULE_SEQUENTIAL) {
        int rc = OHW_OK, total = 0;
        if (hipDeviceGetAttribute(&total, hipDeviceAttributeMultiprocessorCount, e->device) != hipSuccess || total < 2) rc = OHW_E_TRANSCRIBE;
        if (rc == OHW_OK && !e->s_full) rc = ohw_stream_create(e->device, 0, 0, &e->s_full);
        if (e->states.empty()) e->states.assign(1, e->state);
        // LANES: decode batches of up to merge front-end batches (ohw_encode_slice); lane states hold max_batch * merge windows
        const int merge = std::max(1, e->merge);
        const int want_lanes = schedule == OHW_SCHEDULE_LANES ? (int)std::min<int64_t>(e->lanes, n_batches) : 0;
        if (schedule == OHW_SCHEDULE_PIPELINE) {
          while (rc == OHW_OK && (int)e->states.size() < 2) {
            ohw_state* st = nullptr;
            rc = ohw_state_create(e->ctx, e->max_batch, &st);
            if (rc == OHW_OK) { (void)ohw_state_set_packed_encoder(st, e->packed_encoder); (void)ohw_state_set_prefill_chunk(st, e->prefill_chunk); e->states.push_back(st); }
          }
        }
        if (rc == OHW_OK && schedule == OHW_SCHEDULE_PIPELINE && !e->s_enc) {
          if (e->enc_cus >= total) e->enc_cus = std::max(1, total * 3 / 8);   // a smaller device: the same 3 : 5 split
          rc = ohw_stream_create(e->device, 0, e->enc_cus, &e->s_enc);
          if (rc == OHW_OK) rc = ohw_stream_create(e->device, e->enc_cus, total - e->enc_cus, &e->s_dec);
        }
        if (rc == OHW_OK && schedule == OHW_SCHEDULE_LANES) {
          // a lane's state holds what this input can put into one decode batch (cross K/V is 245.76 MB per window at large-v3)
          const int64_t per_lane = std::min<int64_t>(merge, (n_batches + want_lanes - 1) / std::max(1, want_lanes));
          const int need = (int)(e->max_batch * per_lane);
          if (!e->lane_states.empty() && e->lane_capacity < need) {            // a longer input (or another merge factor) than before
            for (ohw_state* st : e->lane_states) ohw_state_free(st);
            e->lane_states.clear();
          }
          if (e->lane_states.empty()) e->lane_capacity = need;
          while (rc == OHW_OK && (int)e->lane_states.size() < want_lanes) {
            ohw_state* st = nullptr;
            rc = ohw_state_create(e->ctx, e->lane_capacity, &st);
            if (rc == OHW_OK) {
              (void)ohw_state_set_packed_encoder(st, e->packed_encoder);
              (void)ohw_state_set_prefill_chunk(st, e->prefill_chunk);
              state_set_graph_max_batch(st, 16);      // see engine.hip: a capture on a lane waits for the other lanes' decodes
              e->lane_states.push_back(st);
            }
          }
          if (rc == OHW_OK && want_lanes >= 2 && (int)e->lane_streams.size() != want_lanes) {
            for (void* ls : e->lane_streams) (void)ohw_stream_destroy(ls);     // another lane count: other CU ranges
            e->lane_streams.clear();
            const int per = std::max(1, total / want_lanes);
            for (int i = 0; rc == OHW_OK && i < want_lanes; ++i) {
              void* ls = nullptr;
              rc = ohw_stream_create(e->device, i * per, per, &ls);
              if (rc == OHW_OK) e->lane_streams.push_back(ls);
            }
          }
        }
        if (rc != OHW_OK) {
          // no CU-masked queues (or no memory for more states) here: one batch after the other from now on
          for (size_t i = 1; i < e->states.size(); ++i) ohw_state_free(e->states[i]);
          e->states.clear();
          for (ohw_state* st : e->lane_states) ohw_state_free(st);
          e->lane_states.clear();
          for (void* ls : e->lane_streams) (void)ohw_stream_destroy(ls);
          e->lane_streams.clear();
          for (void** st : {&e->s_full, &e->s_enc, &e->s_dec}) if (*st) { (void)ohw_stream_destroy(*st); *st = nullptr; }
          e->schedule = schedule = OHW_SCHEDULE_SEQUENTIAL;
        }
      }
      if (schedule == OHW_SCHEDULE_LANES && e->lane_states.empty()) schedule = OHW_SCHEDULE_SEQUENTIAL;
      if (schedule == OHW_SCHEDULE_PIPELINE && (e->states.size() < 2 || !e->s_enc)) schedule = OHW_SCHEDULE_SEQUENTIAL;
      // audio longer than one batch: kernel variants no longer picked from a batch's row count, so a window decodes to the
      // same bits whichever batch (a short last one, a merged one) and schedule it lands in (include/ohw.h)
      struct Invariant {
        ohw_engine* e; bool on;
        void set(bool v) {
          (void)ohw_state_set_batch_invariant(e->state, v);
          for (ohw_state* st : e->states) (void)ohw_state_set_batch_invariant(st, v);
          for (ohw_state* st : e->lane_states) (void)ohw_state_set_batch_invariant(st, v);
        }
        Invariant(ohw_engine* e_, bool on_) : e(e_), on(on_) { if (on) set(true); }
        ~Invariant() { if (on) set(false); }
        // an engine of a pool that aligns: its share may be one batch while the recording is several, and the alignment's path is
        // sensitive to last bits, so the times must not depend on how the windows were dealt
      } invariant(e, n_batches > 1 || (!e->wt_heads.empty() && win_step > 1));
      struct SharedRecording {      // every state of this transcribe reads the recording e->state holds
        ohw_engine* e; bool on;
        SharedRecording(ohw_engine* e_, bool on_) : e(e_), on(on_) {
          if (!on) return;
          for (ohw_state* st : e->states) state_share_recording(st, e->state);
          for (ohw_state* st : e->lane_states) state_share_recording(st, e->state);
        }
        ~SharedRecording() {
          if (!on) return;
          for (ohw_state* st : e->states) if (st != e->state) state_drop_recording(st);
          for (ohw_state* st : e->lane_states) state_drop_recording(st);
        }
      } shared_recording(e, rec_mel);
      // the logit bias of the engine's own state (ohw_state_set_logit_bias on ohw_engine_state(e): the engine's form of
      // whisper.cpp's logits_filter_callback) applies to every state a schedule decodes on, or to none
      {
        const float* bias = state_bias_host(e->state);
        const int V_ = e->ctx->hp.n_vocab;
        auto same = [&](ohw_state* st) {
          if (st == e->state) return;
          const float* b2 = state_bias_host(st);
          if (!bias && !b2) return;
          if (bias && b2 && std::memcmp(bias, b2, (size_t)V_ * sizeof(float)) == 0) return;
          check(ohw_state_set_logit_bias(st, bias, bias ? V_ : 0));
        };
        for (ohw_state* st : e->states) same(st);
        for (ohw_state* st : e->lane_states) same(st);
      }
      apply_ctx();
      auto restore = [&] {
        for (ohw_state* st : e->states) (void)ohw_state_set_stream(st, nullptr);
        for (ohw_state* st : e->lane_states) (void)ohw_state_set_stream(st, nullptr);
        (void)ohw_state_set_stream(e->state, nullptr);
      };
      if (schedule == OHW_SCHEDULE_SEQUENTIAL) {
        Scratch sc(WB, max_tok);
        std::vector<int32_t> ns((size_t)WB);
        for (int64_t bi = 0; bi < n_batches; ++bi) {
          fill_ns(bi, ns);
          mel_windows(e->state, bi * WB, batch_of(bi), ns.data());
          check(ohw_encode(e->state, batch_of(bi)));
          decode_batch(sc, e->state, bi, ns.data());
          collect(sc, batch_of(bi), bi * WB);
        }
      } else if (schedule == OHW_SCHEDULE_PIPELINE) {
        // mel + encoder + cross-K/V of batch i+1 (MFMA-bound) run beside the greedy decode of batch i (HBM- and
        // latency-bound) on disjoint CUs; the first front end and the last decode have the device to themselves
        Scratch sc(e->max_batch, max_tok);
        std::vector<int32_t> ns2[2] = {std::vector<int32_t>((size_t)e->max_batch), std::vector<int32_t>((size_t)e->max_batch)};
        try {
          front(0, e->states[0], e->s_full, ns2[0]);
          void* last_front = e->s_full;
          for (int64_t bi = 0; bi < n_batches; ++bi) {
            const bool more = bi + 1 < n_batches;
            void* dstream = more ? e->s_dec : e->s_full;
            check(ohw_stream_wait(dstream, last_front));            // this batch's cross-K/V before its decode
            if (more) {
              check(ohw_stream_wait(e->s_enc, last_front));
              front(bi + 1, e->states[(bi + 1) & 1], e->s_enc, ns2[(bi + 1) & 1]);
              last_front = e->s_enc;
            }
            check(ohw_state_set_stream(e->states[bi & 1], dstream));
            decode_batch(sc, e->states[bi & 1], bi, ns2[bi & 1].data());
            collect(sc, batch_of(bi), bi * e->max_batch);
          }
        } catch (...) {
          (void)hipDeviceSynchronize();
          restore();
          throw;
        }
        restore();
      } else {
        // LANES: groups of up to L lanes, each lane up to `merge` batches of max_batch windows.  The lanes' front ends (one
        // pass over all of a lane's windows each) run one after the other on every CU (MFMA-bound: nothing to gain from
        // sharing the chip); a lane decodes its windows as ONE batch (the decoder streams its weights once per step whatever
        // its batch); the L decodes run side by side, each on its own CU-masked stream driven by its own host thread - a
        // decode alternates an HBM-bound kernel (cross-attention) with a chain of latency-bound ones, and several together
        // keep HBM busy (tools/decode_overlap_probe.py).  The kernels' arithmetic does not depend on the CU budget or on a
        // window's batch neighbours, so the results equal the sequential schedule's.
        const int L = std::max(1, (int)std::min(e->lane_states.size(), e->lane_streams.empty() ? (size_t)1 : e->lane_streams.size()));
        const int merge = std::max(1, std::min(e->merge, e->lane_capacity / std::max(1, e->max_batch)));
        const int64_t DBw = (int64_t)e->max_batch * merge;                  // capacity of a lane's decode batch, windows
        std::vector<std::unique_ptr<Scratch>> scs;
        std::vector<std::vector<int32_t>> nss((size_t)L, std::vector<int32_t>((size_t)DBw));
        for (int i = 0; i < L; ++i) scs.emplace_back(new Scratch((int)DBw, max_tok));
        try {
          // a group = up to L * merge front-end batches, dealt to the lanes as evenly as they go (4 batches on 4 lanes are 4
          // decode batches of one front end each, not one lane with all four)
          for (int64_t b0 = 0; b0 < n_batches;) {
            const int gb = (int)std::min<int64_t>((int64_t)L * merge, n_batches - b0);
            const int grp = std::min(L, gb);
            std::vector<int64_t> lane_w0((size_t)grp);
            std::vector<int> lane_w((size_t)grp);
            int64_t bnext = b0;
            for (int j = 0; j < grp; ++j) {
              const int mj = gb / grp + (j < gb % grp ? 1 : 0);
              lane_w0[(size_t)j] = bnext * e->max_batch;
              lane_w[(size_t)j] = (int)(std::min<int64_t>(n_win, (bnext + mj) * e->max_batch) - lane_w0[(size_t)j]);
              bnext += mj;
            }
            b0 = bnext;
            for (int j = 0; j < grp; ++j) {
              const int64_t w0 = lane_w0[(size_t)j];
              const int Wd = lane_w[(size_t)j];
              ohw_state* st = e->lane_states[(size_t)j];
              check(ohw_state_set_stream(st, e->s_full));
              // ONE front-end pass over all the lane's windows (its state holds them): the encoder's GEMMs run in rounds of
              // 256 tiles of 256 rows, and 96 windows (563 row tiles) fill their last round where 32 (188) leave it 2/3 empty
              for (int b = 0; b < Wd; ++b) nss[(size_t)j][(size_t)b] = (int32_t)std::min<int64_t>(CHUNK_SAMPLES, n - rec_win(w0 + b) * CHUNK_SAMPLES);
              mel_windows(st, w0, Wd, nss[(size_t)j].data());
              check(ohw_encode(st, Wd));
            }
            if (grp == 1) {
              decode_windows(*scs[0], e->lane_states[0], lane_w0[0], lane_w[0], nss[0].data());
              collect(*scs[0], lane_w[0], lane_w0[0]);
              continue;
            }
            std::vector<std::string> errs((size_t)grp);
            std::vector<std::thread> th;
            // the host waits for the group's front ends before the lane threads start: lanes that begin to enqueue their
            // decode while the front ends still run cost 6 % of a step in bench.py (283.9 against 262 - 268 ms)
            check(ohw_stream_sync(e->s_full));
            for (int j = 0; j < grp; ++j) {
              check(ohw_stream_wait(e->lane_streams[(size_t)j], e->s_full));
              check(ohw_state_set_stream(e->lane_states[(size_t)j], e->lane_streams[(size_t)j]));
            }
            for (int j = 0; j < grp; ++j)
              th.emplace_back([&, j] {
                try {
                  decode_windows(*scs[(size_t)j], e->lane_states[(size_t)j], lane_w0[(size_t)j], lane_w[(size_t)j], nss[(size_t)j].data());
                } catch (const std::exception& ex) {
                  errs[(size_t)j] = ex.what()[0] ? ex.what() : "unknown error";
                }
              });
            {
              ApiRelease wait_only;        // the lanes take the library's gate themselves (exclusively while one captures its graph)
              for (auto& t : th) t.join();
            }
            for (int j = 0; j < grp; ++j) if (!errs[(size_t)j].empty()) throw Error(OHW_E_TRANSCRIBE, errs[(size_t)j]);
            for (int j = 0; j < grp; ++j) {
              check(ohw_stream_wait(e->s_full, e->lane_streams[(size_t)j]));
              collect(*scs[(size_t)j], lane_w[(size_t)j], lane_w0[(size_t)j]);
            }
          }
        } catch (...) {
          (void)hipDeviceSynchronize();
          restore();
          throw;
        }
        restore();
      }
    }
}

}  // namespace ohw

extern "C" {

const char* ohw_lang_id_to_code(int32_t id) { return (id >= 0 && id < 99) ? kLangs[id] : "unknown"; }

int32_t ohw_lang_code_to_id(const char* code) {
  if (!code) return -1;
  for (int i = 0; i < 99; ++i)
    if (std::strcmp(code, kLangs[i]) == 0) return i;
  return -1;
}

int ohw_validate_audio(const float* samples, int64_t n, uint32_t sample_rate, ohw_audio_info* info) {
  if (!info) return OHW_E_INVALID_ARG;
  std::memset(info, 0, sizeof *info);
  auto fail = [&](int code) { info->error = code; return OHW_E_VALIDATION; };
  if (n <= 0 || !samples) return fail(OHW_AUDIO_EMPTY);                      // validation.rs:51-53
  if (sample_rate != 16000u) return fail(OHW_AUDIO_BAD_RATE);               // :56-61
  const float duration = (float)n / (float)sample_rate;                     // :64
  info->duration_secs = duration;
  info->sample_count = n;
  if (duration > 7200.0f) return fail(OHW_AUDIO_TOO_LONG);                  // :67-72 (before the scan)
  if (duration < 0.1f) return fail(OHW_AUDIO_TOO_SHORT);                    // :74-79
  float mn = 3.40282347e+38f, mx = -3.40282347e+38f;
  double ss = 0.0;
  int64_t n_nan = 0, n_inf = 0;
  for (int64_t i = 0; i < n; ++i) {                                         // :88-98
    const float v = samples[i];
    if (std::isnan(v)) ++n_nan;
    else if (std::isinf(v)) ++n_inf;
    else { mn = std::min(mn, v); mx = std::max(mx, v); ss += (double)v * (double)v; }
  }
  info->nan_count = n_nan;
  info->inf_count = n_inf;
  if (n_nan > 0) return fail(OHW_AUDIO_NAN);                                // :100-102
  if (n_inf > 0) return fail(OHW_AUDIO_INF);                                // :104-106
  info->min_value = mn;
  info->max_value = mx;
  info->rms = (float)std::sqrt(ss / (double)n);                             // :109
  info->error = OHW_AUDIO_OK;
  return OHW_OK;
}

// Host-side logits filter: whisper.cpp's whisper_process_logits with the defaults the reference inherits
// (SURVEY.md A4.6, Appendix A).  Same rule order as the device sampler in decode.hip.  Masks `logits` in place
// (timestamp-mass rule included) and returns the log-sum-exp taken BEFORE that rule, as whisper.cpp's logprobs are.
static float filter_logits(const ohw_ctx* ctx, const ohw_sample_params* p, float* logits, const int32_t* cur, int n_cur) {
  const ohw_special_tokens& t = ctx->tok;
  const int V = ctx->hp.n_vocab;
  const float NEG = -INFINITY;
  const bool is_initial = n_cur == 0;
  if (p->suppress_blank && is_initial) {
    logits[t.eot] = NEG;
    if (t.blank >= 0) logits[t.blank] = NEG;
  }
  logits[t.no_timestamps] = NEG;
  logits[t.sot] = NEG; logits[t.nosp] = NEG; logits[t.translate] = NEG; logits[t.transcribe] = NEG;
  logits[t.prev] = NEG; logits[t.solm] = NEG;
  for (int i = 0; i < t.n_langs; ++i) logits[t.sot + 1 + i] = NEG;
  if (p->force_len > 0 && n_cur < p->force_len) logits[t.eot] = NEG;
  if (p->no_timestamps) {
    for (int i = t.timestamp_begin; i < V; ++i) logits[i] = NEG;
  } else {
    const bool last_ts = n_cur > 0 && cur[n_cur - 1] >= t.timestamp_begin;
    const bool penult_ts = n_cur < 2 || cur[n_cur - 2] >= t.timestamp_begin;
    if (last_ts) {
      if (penult_ts) { for (int i = t.timestamp_begin; i < V; ++i) logits[i] = NEG; }
      else { for (int i = 0; i < t.eot; ++i) logits[i] = NEG; }
    }
    if (is_initial && p->max_initial_ts > 0)
      for (int i = t.timestamp_begin + p->max_initial_ts + 1; i < V; ++i) logits[i] = NEG;
    int last_seen = -1;
    for (int i = n_cur - 1; i >= 0; --i) if (cur[i] >= t.timestamp_begin) { last_seen = cur[i]; break; }
    if (last_seen >= 0) for (int i = t.timestamp_begin; i < last_seen; ++i) logits[i] = NEG;
  }
  float mx = NEG;
  for (int i = 0; i < V; ++i) mx = std::max(mx, logits[i]);
  double sum = 0.0, ts_sum = 0.0;
  float text_max = NEG;
  for (int i = 0; i < V; ++i) {
    if (!(logits[i] > NEG)) continue;
    const double e = std::exp((double)(logits[i] - mx));
    sum += e;
    if (i >= t.timestamp_begin) ts_sum += e; else text_max = std::max(text_max, logits[i]);
  }
  const float lse = mx + (float)std::log(sum);
  if (!p->no_timestamps && ts_sum > 0.0) {
    const float ts_lp = mx + (float)std::log(ts_sum) - lse;
    if (ts_lp > text_max - lse) for (int i = 0; i < t.timestamp_begin; ++i) logits[i] = NEG;
  }
  return lse;
}

int32_t ohw_sample_greedy_host(const ohw_ctx* ctx, const ohw_sample_params* p, float* logits, const int32_t* cur, int n_cur,
                               float* logprob_out) {
  if (!ctx || !p || !logits) return -1;
  const float lse = filter_logits(ctx, p, logits, cur, n_cur);
  const int V = ctx->hp.n_vocab;
  int best = 0;
  float bv = -INFINITY;
  for (int i = 0; i < V; ++i) if (logits[i] > bv) { bv = logits[i]; best = i; }
  if (logprob_out) *logprob_out = bv - lse;
  return best;
}

// whisper.cpp's decoders draw with std::mt19937 (seeded 0 once per whisper_full call) through
// std::discrete_distribution over exp(logprobs): whisper_sample_token with best = false
struct ohw_rng { std::mt19937 gen; };
ohw_rng* ohw_rng_new(uint32_t seed) { return new (std::nothrow) ohw_rng{std::mt19937(seed)}; }
void ohw_rng_free(ohw_rng* r) { delete r; }

int32_t ohw_sample_host(const ohw_ctx* ctx, const ohw_sample_params* p, float* logits, const int32_t* cur, int n_cur, float temperature,
                        ohw_rng* rng, float* logprob_out, float* no_speech_prob_out) {
  if (!ctx || !p || !logits) return -1;
  const int V = ctx->hp.n_vocab;
  if (temperature > 0.0f) for (int i = 0; i < V; ++i) logits[i] /= temperature;
  if (no_speech_prob_out && n_cur == 0) {
    float mx = -INFINITY;
    for (int i = 0; i < V; ++i) mx = std::max(mx, logits[i]);
    double sum = 0.0;
    for (int i = 0; i < V; ++i) sum += std::exp((double)(logits[i] - mx));
    *no_speech_prob_out = (float)std::exp((double)(logits[ctx->tok.nosp] - mx) - std::log(sum));
  }
  if (!(temperature > 0.0f)) return ohw_sample_greedy_host(ctx, p, logits, cur, n_cur, logprob_out);
  if (!rng) return -1;
  const float lse = filter_logits(ctx, p, logits, cur, n_cur);
  std::vector<float> probs((size_t)V);
  for (int i = 0; i < V; ++i) probs[(size_t)i] = logits[i] > -INFINITY ? std::exp(logits[i] - lse) : 0.0f;
  std::discrete_distribution<> dist(probs.begin(), probs.end());
  const int id = dist(rng->gen);
  if (logprob_out) *logprob_out = logits[id] - lse;
  return id;
}

// a draw of std::discrete_distribution<int> in libstdc++ is exactly one std::generate_canonical<double, 53> (two engine
// outputs, the lower_bound of it in the normalised partial sums): the stream position of every draw is known in advance
int ohw_rng_uniforms(const ohw_rng* rng, int n, double* out) {
  if (!rng || n < 0 || (n > 0 && !out)) return OHW_E_INVALID_ARG;
  std::mt19937 g = rng->gen;
  for (int i = 0; i < n; ++i) out[i] = std::generate_canonical<double, std::numeric_limits<double>::digits>(g);
  return OHW_OK;
}

int ohw_rng_discard_draws(ohw_rng* rng, int n) {
  if (!rng || n < 0) return OHW_E_INVALID_ARG;
  for (int i = 0; i < n; ++i) (void)std::generate_canonical<double, std::numeric_limits<double>::digits>(rng->gen);
  return OHW_OK;
}

int ohw_detect_language(ohw_state* st, int batch, int32_t* lang_ids_out, float* lang_probs_out) {
  return guard([&] {
    if (!st || !lang_ids_out || batch < 1) throw Error(OHW_E_INVALID_ARG, "bad argument");
    const ohw_ctx* ctx = ohw_state_ctx(st);
    const ohw_special_tokens& t = ctx->tok;
    if (ctx->hp.n_vocab < 51865) throw Error(OHW_E_INVALID_ARG, "language detection needs a multilingual model");
    const int V = ctx->hp.n_vocab, nl = t.n_langs;
    std::vector<int32_t> toks((size_t)batch, t.sot), past((size_t)batch, 0);
    std::vector<float> logits((size_t)batch * V);
    const int rc = ohw_decode(st, toks.data(), 1, past.data(), batch, logits.data());
    if (rc != OHW_OK) throw Error(rc, g_last_error);
    for (int b = 0; b < batch; ++b) {
      const float* lg = logits.data() + (size_t)b * V + t.sot + 1;
      float mx = -INFINITY;
      int best = 0;
      for (int i = 0; i < nl; ++i) if (lg[i] > mx) { mx = lg[i]; best = i; }
      lang_ids_out[b] = best;
      if (lang_probs_out) {
        double sum = 0.0;
        for (int i = 0; i < nl; ++i) sum += std::exp((double)(lg[i] - mx));
        for (int i = 0; i < nl; ++i) lang_probs_out[(size_t)b * nl + i] = (float)(std::exp((double)(lg[i] - mx)) / sum);
      }
    }
  });
}

// the definition of lang_pick_kernel's result (decode.hip): the first maximum of the raw language columns and their soft-max
// in fp32 (ohw_detect_language above keeps its double sums: its results must not move)
int ohw_lang_pick_host(const float* row, const ohw_special_tokens* tok, int32_t* id, float* probs) {
  if (!row || !tok || !id || tok->n_langs < 1) return OHW_E_INVALID_ARG;
  const float* lg = row + tok->sot + 1;
  const int nl = tok->n_langs;
  float mx = -INFINITY;
  int best = 0;
  for (int i = 0; i < nl; ++i) if (lg[i] > mx) { mx = lg[i]; best = i; }
  *id = best;
  if (probs) {
    float sum = 0.f;
    for (int i = 0; i < nl; ++i) sum += std::exp(lg[i] - mx);
    for (int i = 0; i < nl; ++i) probs[i] = std::exp(lg[i] - mx) / sum;
  }
  return OHW_OK;
}

int ohw_engine_new(const char* model_path, const char* language, int translate, int use_gpu, int device, int dtype, int max_batch,
                   ohw_engine** out) {
  return guard([&] {
    if (!out) throw Error(OHW_E_INVALID_ARG, "out is null");
    *out = nullptr;
    struct stat sb;
    if (!model_path || stat(model_path, &sb) != 0) {
      // reference :141-154: the model name is the file stem without "ggml-"
      std::string stem = model_path ? model_path : "";
      const size_t slash = stem.find_last_of('/');
      if (slash != std::string::npos) stem = stem.substr(slash + 1);
      const size_t dot = stem.find_last_of('.');
      if (dot != std::string::npos) stem = stem.substr(0, dot);
      std::string name = stem.rfind("ggml-", 0) == 0 ? stem.substr(5) : "unknown";
      throw Error(OHW_E_MODEL_NOT_FOUND, std::string("Model not found at ") + (model_path ? model_path : "(null)") +
                                             ". Run 'openhush model download " + name + "'");
    }
    if (!use_gpu)
      throw Error(OHW_E_NO_GPU, "device = \"cpu\": this engine has no CPU path (set [transcription] device to \"hip:N\")");
    const std::string lang = language ? language : "auto";
    if (lang != "auto" && ohw_lang_code_to_id(lang.c_str()) < 0)
      throw Error(OHW_E_LOAD_FAILED, "unknown language code '" + lang + "'");
    ohw_ctx* ctx = nullptr;
    int rc = ohw_ctx_create(model_path, device, dtype, &ctx);
    if (rc != OHW_OK) throw Error(rc == OHW_E_MODEL_NOT_FOUND ? rc : (rc == OHW_E_NO_GPU || rc == OHW_E_OOM ? rc : OHW_E_LOAD_FAILED),
                                  "Failed to load model: " + g_last_error);
    std::unique_ptr<ohw_engine> e;
    try {
      e.reset(engine_wrap_ctx(ctx, lang, translate != 0, max_batch, device));
    } catch (...) {
      ohw_ctx_free(ctx);
      throw;
    }
    *out = e.release();
  });
}

void ohw_engine_free(ohw_engine* e) {
  if (!e) return;
  ohw_state_free(e->state);
  for (size_t i = 1; i < e->states.size(); ++i) ohw_state_free(e->states[i]);
  for (ohw_state* st : e->lane_states) ohw_state_free(st);
  for (void* ls : e->lane_streams) (void)ohw_stream_destroy(ls);
  for (void* st : {e->s_full, e->s_enc, e->s_dec}) if (st) (void)ohw_stream_destroy(st);
  ohw_ctx_free(e->ctx);
  delete e;
}

ohw_state* ohw_engine_state(ohw_engine* e) { return e ? e->state : nullptr; }
ohw_ctx* ohw_engine_ctx(ohw_engine* e) { return e ? e->ctx : nullptr; }

int ohw_engine_transcribe(ohw_engine* e, const float* samples, int64_t n, uint32_t sample_rate, char* text_buf, size_t text_cap,
                          char* language_out, uint64_t* duration_ms, ohw_audio_info* info_out) {
  return guard([&] {
    if (!e) throw Error(OHW_E_INVALID_ARG, "engine is null");
    ohw_audio_info info;
    const int vrc = ohw_validate_audio(samples, n, sample_rate, &info);   // reference :206
    if (info_out) *info_out = info;
    if (vrc != OHW_OK) {
      static const char* const names[] = {"ok", "Audio is empty (no samples)", "Unexpected sample rate", "Audio too long", "Audio too short",
                                          "Audio contains NaN values", "Audio contains infinite values"};
      throw Error(OHW_E_VALIDATION, std::string("Audio validation failed: ") + names[info.error]);
    }
    const auto t0 = std::chrono::steady_clock::now();                       // reference :231
    std::string text;
    engine_transcribe_core(e, samples, n, &text);
    // reference :282-283: trim
    const size_t b0 = text.find_first_not_of(" \t\r\n");
    const size_t b1 = text.find_last_not_of(" \t\r\n");
    text = b0 == std::string::npos ? std::string() : text.substr(b0, b1 - b0 + 1);
    e->last_text = text;
    trim_spans(e->last_words, b0 == std::string::npos ? 0 : b0, text.size());       // the spans index the trimmed text
    trim_spans(e->last_segments, b0 == std::string::npos ? 0 : b0, text.size());
    if (text_buf && text_cap > 0) {
      const size_t ncopy = std::min(text.size(), text_cap - 1);
      std::memcpy(text_buf, text.data(), ncopy);
      text_buf[ncopy] = 0;
    }
    if (language_out) {
      // reference :288-296: "auto" reports the state's language id (whisper.cpp default "en" -> 0; the detected one with
      // ohw_engine_set_detect_language)
      const std::string lang = e->language == "auto" ? ohw_lang_id_to_code(e->last_lang_id) : e->language;
      std::strncpy(language_out, lang.c_str(), 7);
      language_out[7] = 0;
    }
    if (duration_ms)
      *duration_ms = (uint64_t)std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count();
  });
}

int ohw_batch_plan(const int64_t* n_samples, int n_recs, int max_batch, int audio_ctx_setting, int32_t* order_out, int32_t* ctx_out,
                   int32_t* envelope_out) {
  return guard([&] {
    if (!n_samples || n_recs < 1 || max_batch < 1 || !order_out || !ctx_out || !envelope_out) throw Error(OHW_E_INVALID_ARG, "batch_plan: bad argument");
    if (audio_ctx_setting < -1 || audio_ctx_setting > 1500) throw Error(OHW_E_INVALID_ARG, "batch_plan: audio_ctx must be 0, 1..1500 or -1 (auto)");
    for (int i = 0; i < n_recs; ++i) {
      const int64_t n = n_samples[i];
      if (n < 0 || n > CHUNK_SAMPLES)
        throw Error(OHW_E_INVALID_ARG, "recording " + std::to_string(i) + " holds " + std::to_string(n) + " samples: a recording of a batch is at most one 30 s window (480000)");
      if (audio_ctx_setting > 0 && n > (int64_t)audio_ctx_setting * 320)
        throw Error(OHW_E_INVALID_ARG, "audio_ctx " + std::to_string(audio_ctx_setting) + " covers " + std::to_string((int64_t)audio_ctx_setting * 320) +
                                           " samples, recording " + std::to_string(i) + " holds " + std::to_string(n));
      ctx_out[i] = audio_ctx_setting > 0 ? audio_ctx_setting : audio_ctx_setting < 0 ? ohw_audio_ctx_for(n) : 1500;
    }
    for (int i = 0; i < n_recs; ++i) order_out[i] = i;
    std::stable_sort(order_out, order_out + n_recs, [&](int32_t a, int32_t b) { return n_samples[a] > n_samples[b]; });
    for (int j = 0; j * max_batch < n_recs; ++j) {
      int32_t m = 0;
      for (int k = j * max_batch; k < std::min(n_recs, (j + 1) * max_batch); ++k) m = std::max(m, ctx_out[order_out[k]]);
      envelope_out[j] = m;
    }
  });
}

int ohw_engine_transcribe_batch(ohw_engine* e, const ohw_audio_span* recs, int n_recs, uint32_t sample_rate) {
  return ohw_engine_transcribe_batch_lang(e, recs, nullptr, n_recs, sample_rate);
}

int ohw_engine_set_word_timestamps(ohw_engine* e, const ohw_align_head* heads, int n) {
  return guard([&] {
    if (!e) throw Error(OHW_E_INVALID_ARG, "engine is null");
    if (!heads || n == 0) {
      // off: every state of the engine that may have aligned gives its buffers back
      e->wt_heads.clear();
      (void)ohw_state_set_align_heads(e->state, nullptr, 0);
      for (ohw_state* st : e->states) if (st != e->state) (void)ohw_state_set_align_heads(st, nullptr, 0);
      for (ohw_state* st : e->lane_states) (void)ohw_state_set_align_heads(st, nullptr, 0);
      return;
    }
    // checked here against the model, as ohw_state_set_align_heads checks it; a state allocates when it first aligns
    const ohw_hparams& hp = e->ctx->hp;
    if (n < 0 || n > OHW_ALIGN_MAX_HEADS)
      throw Error(OHW_E_INVALID_ARG, "set_word_timestamps: " + std::to_string(n) + " heads, at most " + std::to_string(OHW_ALIGN_MAX_HEADS) + " (OHW_ALIGN_MAX_HEADS)");
    for (int i = 0; i < n; ++i)
      if (heads[i].layer < 0 || heads[i].layer >= hp.n_text_layer || heads[i].head < 0 || heads[i].head >= hp.n_text_head)
        throw Error(OHW_E_INVALID_ARG, "set_word_timestamps: entry " + std::to_string(i) + " (layer " + std::to_string(heads[i].layer) + ", head " +
                                           std::to_string(heads[i].head) + ") is outside the model (" + std::to_string(hp.n_text_layer) + " layers, " +
                                           std::to_string(hp.n_text_head) + " heads)");
    e->wt_heads.assign(heads, heads + n);
  });
}

static int spans_out(const std::vector<ohw_token_time>& tt, const std::vector<ohw_span_time>& w, const std::vector<ohw_span_time>& s,
                     const ohw_token_time** tp, int* tn, const ohw_span_time** wp, int* wn, const ohw_span_time** sp_, int* sn) {
  if (tp) *tp = tt.data();
  if (tn) *tn = (int)tt.size();
  if (wp) *wp = w.data();
  if (wn) *wn = (int)w.size();
  if (sp_) *sp_ = s.data();
  if (sn) *sn = (int)s.size();
  return OHW_OK;
}
int ohw_engine_last_token_times(ohw_engine* e, const ohw_token_time** t, int* n) {
  if (!e || !t || !n) return OHW_E_INVALID_ARG;
  return spans_out(e->last_token_times, e->last_words, e->last_segments, t, n, nullptr, nullptr, nullptr, nullptr);
}
int ohw_engine_last_words(ohw_engine* e, const ohw_span_time** w, int* n) {
  if (!e || !w || !n) return OHW_E_INVALID_ARG;
  return spans_out(e->last_token_times, e->last_words, e->last_segments, nullptr, nullptr, w, n, nullptr, nullptr);
}
int ohw_engine_last_segments(ohw_engine* e, const ohw_span_time** s, int* n) {
  if (!e || !s || !n) return OHW_E_INVALID_ARG;
  return spans_out(e->last_token_times, e->last_words, e->last_segments, nullptr, nullptr, nullptr, nullptr, s, n);
}
int ohw_engine_batch_times(ohw_engine* e, int i, const ohw_token_time** token_times, int* n_token_times, const ohw_span_time** words, int* n_words,
                           const ohw_span_time** segments, int* n_segments) {
  return guard([&] {
    if (!e) throw Error(OHW_E_INVALID_ARG, "engine is null");
    if (i < 0 || i >= (int)e->batch_records.size()) throw Error(OHW_E_INVALID_ARG, "batch_times: no recording " + std::to_string(i) + " in the last transcribe_batch");
    const ohw_engine::BatchRecord& r = e->batch_records[(size_t)i];
    spans_out(r.token_times, r.words, r.segments, token_times, n_token_times, words, n_words, segments, n_segments);
  });
}

int ohw_word_starts_host(const char* bytes, const int32_t* lens, int n, int32_t* starts_out) {
  return guard([&] {
    if (n < 0 || (n > 0 && (!bytes || !lens || !starts_out))) throw Error(OHW_E_INVALID_ARG, "word_starts: bad argument");
    size_t off = 0;
    for (int i = 0; i < n; ++i) {
      if (lens[i] < 0) throw Error(OHW_E_INVALID_ARG, "word_starts: token " + std::to_string(i) + " has a negative length");
      bool start = i == 0;
      if (!start && lens[i] > 0 && bytes[off] == ' ') {
        // do the bytes in front end on a complete UTF-8 sequence?  walk back over continuation bytes to the lead byte
        size_t k = off, cont = 0;
        while (k > 0 && cont < 3 && ((unsigned char)bytes[k - 1] & 0xC0) == 0x80) { --k; ++cont; }
        if (k == 0) start = cont == 0;
        else {
          const unsigned char lead = (unsigned char)bytes[k - 1];
          const size_t want = lead < 0x80 ? 0 : (lead & 0xE0) == 0xC0 ? 1 : (lead & 0xF0) == 0xE0 ? 2 : (lead & 0xF8) == 0xF0 ? 3 : 99;
          start = want == cont;
        }
      }
      starts_out[i] = start ? 1 : 0;
      off += (size_t)lens[i];
    }
  });
}

int ohw_segments_host(const int32_t* tokens, int n, const ohw_special_tokens* tok, float t_off, float t_end, ohw_token_span* out, int cap) {
  if (n < 0 || (n > 0 && !tokens) || !tok || cap < 0 || (cap > 0 && !out)) return OHW_E_INVALID_ARG;
  int count = 0, first = -1;
  float t0 = t_off;
  auto put = [&](int end, float t1) {
    if (count < cap) out[count] = ohw_token_span{first, end, t0, t1};
    ++count;
    first = -1;
  };
  for (int i = 0; i < n; ++i) {
    const int32_t id = tokens[i];
    if (id >= tok->timestamp_begin) {
      const float t = t_off + (float)(id - tok->timestamp_begin) * 0.02f;
      if (first >= 0) put(i, t);
      t0 = t;
    } else if (id < tok->eot && first < 0) first = i;
  }
  if (first >= 0) put(n, t_end);
  return count;
}

int ohw_engine_set_detect_language(ohw_engine* e, int on) {
  if (!e) return OHW_E_INVALID_ARG;
  e->detect_language = on != 0;
  return OHW_OK;
}

int ohw_engine_last_language(ohw_engine* e, int32_t* id, float* prob) {
  if (!e) return OHW_E_INVALID_ARG;
  if (id) *id = e->last_lang_id;
  if (prob) *prob = e->last_lang_prob;
  return OHW_OK;
}

int ohw_engine_transcribe_batch_lang(ohw_engine* e, const ohw_audio_span* recs, const int32_t* lang_ids, int n_recs, uint32_t sample_rate) {
  return guard([&] {
    if (!e || !recs || n_recs < 1) throw Error(OHW_E_INVALID_ARG, "transcribe_batch: null engine or no recordings");
    if (e->window_mode != OHW_WINDOW_FIXED) throw Error(OHW_E_INVALID_ARG, "transcribe_batch: recordings are cut as OHW_WINDOW_FIXED cuts; set that window mode");
    e->batch_records.clear();
    for (int i = 0; i < n_recs; ++i) {
      ohw_audio_info info;
      if (ohw_validate_audio(recs[i].samples, recs[i].n, sample_rate, &info) != OHW_OK) {
        static const char* const names[] = {"ok", "Audio is empty (no samples)", "Unexpected sample rate", "Audio too long", "Audio too short",
                                            "Audio contains NaN values", "Audio contains infinite values"};
        throw Error(OHW_E_VALIDATION, "Audio validation failed for recording " + std::to_string(i) + ": " + names[info.error]);
      }
    }
    engine_transcribe_core(e, nullptr, 0, nullptr, 0, 1, recs, n_recs, lang_ids);
  });
}

// ---- ohw_seek_sched_*: host only -------------------------------------------------------------------------------------------
int ohw_seek_sched_new(const int64_t* n_samples, int n_recs, int max_batch, ohw_seek_sched** out) {
  return guard([&] {
    if (!n_samples || n_recs < 1 || max_batch < 1 || !out) throw Error(OHW_E_INVALID_ARG, "seek_sched: bad argument");
    *out = nullptr;
    std::unique_ptr<ohw_seek_sched> s(new ohw_seek_sched());
    s->max_batch = max_batch;
    s->seek.assign((size_t)n_recs, 0);
    s->seek_end.resize((size_t)n_recs);
    for (int i = 0; i < n_recs; ++i) {
      if (n_samples[i] < 0 || n_samples[i] > (int64_t)7200 * 16000)
        throw Error(OHW_E_INVALID_ARG, "seek_sched: recording " + std::to_string(i) + " holds " + std::to_string(n_samples[i]) + " samples (0 .. two hours)");
      s->seek_end[(size_t)i] = mel_frames(n_samples[i]);
      if (s->live(i)) s->waiting.push_back(i);
    }
    std::stable_sort(s->waiting.begin(), s->waiting.end(), [&](int32_t a, int32_t b) { return n_samples[a] > n_samples[b]; });
    s->slot_rec.assign((size_t)max_batch, -1);
    s->slot_fresh.assign((size_t)max_batch, 0);
    *out = s.release();
  });
}

int ohw_seek_sched_round(ohw_seek_sched* s, int32_t* rec_out, int32_t* slot_out, int32_t* seek_out, int32_t* fresh_out) {
  if (!s || !rec_out || !slot_out || !seek_out || !fresh_out) { g_last_error = "seek_sched_round: null argument"; return -1; }
  // free slots, lowest first, go to the waiting recordings in their order
  for (int k = 0; k < s->max_batch && s->next_waiting < s->waiting.size(); ++k)
    if (s->slot_rec[(size_t)k] < 0) { s->slot_rec[(size_t)k] = s->waiting[s->next_waiting++]; s->slot_fresh[(size_t)k] = 1; }
  s->round_rec.clear();
  int B = 0;
  for (int k = 0; k < s->max_batch; ++k) {
    const int r = s->slot_rec[(size_t)k];
    if (r < 0) continue;
    rec_out[B] = r; slot_out[B] = k; seek_out[B] = s->seek[(size_t)r]; fresh_out[B] = s->slot_fresh[(size_t)k];
    s->slot_fresh[(size_t)k] = 0;
    s->round_rec.push_back(r);
    ++B;
  }
  return B;
}

int ohw_seek_sched_advance(ohw_seek_sched* s, int b, int seek_delta) {
  return guard([&] {
    if (!s) throw Error(OHW_E_INVALID_ARG, "seek_sched_advance: null scheduler");
    if (b < 0 || b >= (int)s->round_rec.size() || s->round_rec[(size_t)b] < 0)
      throw Error(OHW_E_INVALID_ARG, "seek_sched_advance: no entry " + std::to_string(b) + " to advance in the last round");
    const int r = s->round_rec[(size_t)b];
    s->round_rec[(size_t)b] = -1;             // one advance per entry and round
    s->seek[(size_t)r] += seek_delta > 0 ? seek_delta : 3000;
    if (!s->live(r))
      for (auto& sr : s->slot_rec) if (sr == r) sr = -1;
  });
}

void ohw_seek_sched_free(ohw_seek_sched* s) { delete s; }

int ohw_engine_transcribe_long_batch(ohw_engine* e, const ohw_audio_span* recs, const int32_t* lang_ids, int n_recs, uint32_t sample_rate) {
  return guard([&] {
    if (!e || !recs || n_recs < 1) throw Error(OHW_E_INVALID_ARG, "transcribe_long_batch: null engine or no recordings");
    e->batch_records.clear();
    for (int i = 0; i < n_recs; ++i) {
      ohw_audio_info info;
      if (ohw_validate_audio(recs[i].samples, recs[i].n, sample_rate, &info) != OHW_OK) {
        static const char* const names[] = {"ok", "Audio is empty (no samples)", "Unexpected sample rate", "Audio too long", "Audio too short",
                                            "Audio contains NaN values", "Audio contains infinite values"};
        throw Error(OHW_E_VALIDATION, "Audio validation failed for recording " + std::to_string(i) + ": " + names[info.error]);
      }
      if (recs[i].n > (int64_t)7200 * 16000)
        throw Error(OHW_E_INVALID_ARG, "transcribe_long_batch: recording " + std::to_string(i) + " is longer than two hours, the limit of a recording slot");
    }
    // the seek loop whatever ohw_engine_set_window_mode says: the per-window bookkeeping reads the mode
    struct Mode { ohw_engine* e; int was; ~Mode() { e->window_mode = was; } } mode{e, e->window_mode};
    e->window_mode = OHW_WINDOW_SEEK;
    engine_transcribe_core(e, nullptr, 0, nullptr, 0, 1, recs, n_recs, lang_ids, true);
  });
}

int ohw_engine_long_batch_quality(ohw_engine* e, int i, const ohw_window_quality** q, int* n_windows) {
  return guard([&] {
    if (!e || !q || !n_windows) throw Error(OHW_E_INVALID_ARG, "long_batch_quality: null argument");
    if (i < 0 || i >= (int)e->batch_records.size()) throw Error(OHW_E_INVALID_ARG, "long_batch_quality: no recording " + std::to_string(i) + " in the last batch call");
    const ohw_engine::BatchRecord& r = e->batch_records[(size_t)i];
    *q = r.qualities.data();
    *n_windows = (int)r.qualities.size();
  });
}

int ohw_engine_batch_result(ohw_engine* e, int i, const char** text, size_t* text_len, const int32_t** tokens, int* n_tokens,
                            const ohw_window_quality** quality, char* language_out) {
  return guard([&] {
    if (!e) throw Error(OHW_E_INVALID_ARG, "engine is null");
    if (i < 0 || i >= (int)e->batch_records.size()) throw Error(OHW_E_INVALID_ARG, "batch_result: no recording " + std::to_string(i) + " in the last transcribe_batch");
    const ohw_engine::BatchRecord& r = e->batch_records[(size_t)i];
    if (text) *text = r.text.c_str();
    if (text_len) *text_len = r.text.size();
    if (tokens) *tokens = r.tokens.data();
    if (n_tokens) *n_tokens = (int)r.tokens.size();
    if (quality) *quality = r.qualities.empty() ? &r.quality : r.qualities.data();     // long batch: one record per window
    if (language_out) {
      const std::string lang = r.lang_id >= 0 ? ohw_lang_id_to_code(r.lang_id) : e->language == "auto" ? ohw_lang_id_to_code(0) : e->language;
      std::strncpy(language_out, lang.c_str(), 7);
      language_out[7] = 0;
    }
  });
}

void ohw_default_decode_policy(ohw_decode_policy* q) {
  if (!q) return;
  q->temperature_inc = 0.2f; q->entropy_thold = 2.4f; q->logprob_thold = -1.0f; q->no_speech_thold = 0.6f;
}

int ohw_engine_set_decode_policy(ohw_engine* e, const ohw_decode_policy* q) {
  if (!e || !q) return OHW_E_INVALID_ARG;
  e->policy = *q;
  return OHW_OK;
}

int ohw_engine_set_fallback_device(ohw_engine* e, int on) {
  if (!e) return OHW_E_INVALID_ARG;
  e->fallback_device = on != 0;
  return OHW_OK;
}

int ohw_engine_last_trace(ohw_engine* e, const int32_t** data, int* n) {
  if (!e || !data || !n) return OHW_E_INVALID_ARG;
  *data = e->last_trace.data();
  *n = (int)e->last_trace.size();
  return OHW_OK;
}

int ohw_engine_last_text(ohw_engine* e, const char** text, size_t* len) {
  if (!e || !text) return OHW_E_INVALID_ARG;
  *text = e->last_text.c_str();
  if (len) *len = e->last_text.size();
  return OHW_OK;
}

int ohw_engine_last_quality(ohw_engine* e, const ohw_window_quality** q, int* n_windows) {
  if (!e || !q || !n_windows) return OHW_E_INVALID_ARG;
  *q = e->last_quality.data();
  *n_windows = (int)e->last_quality.size();
  return OHW_OK;
}

int ohw_engine_set_schedule(ohw_engine* e, int schedule, int lanes, int merge) {
  if (!e || schedule < OHW_SCHEDULE_SEQUENTIAL || schedule > OHW_SCHEDULE_LANES || lanes < 0 || lanes > 16 || merge < 0 || merge > 8) return OHW_E_INVALID_ARG;
  e->schedule = schedule;
  if (lanes > 0) e->lanes = lanes;
  if (merge > 0) e->merge = std::min(merge, std::max(1, 256 / e->max_batch));
  return OHW_OK;
}

int ohw_engine_set_audio_ctx(ohw_engine* e, int n) {
  if (!e || n < -1 || n > e->ctx->hp.n_audio_ctx) return OHW_E_INVALID_ARG;
  e->audio_ctx = n == e->ctx->hp.n_audio_ctx ? 0 : n;
  return OHW_OK;
}

int ohw_engine_set_initial_prompt_tokens(ohw_engine* e, const int32_t* tokens, int n) {
  return guard([&] {
    if (!e || n < 0 || (n > 0 && !tokens)) throw Error(OHW_E_INVALID_ARG, "initial_prompt: bad argument");
    for (int i = 0; i < n; ++i)
      if (tokens[i] < 0 || tokens[i] >= e->ctx->hp.n_vocab)
        throw Error(OHW_E_INVALID_ARG, "initial_prompt: token " + std::to_string(i) + " = " + std::to_string(tokens[i]) + " is outside the vocabulary");
    std::vector<int32_t> kept((size_t)std::max(n, 1));
    const int k = n > 0 ? ohw_prompt_clip_host(tokens, n, e->ctx->hp.n_text_ctx, kept.data()) : 0;
    if (k < 0) throw Error(OHW_E_INVALID_ARG, "initial_prompt: " + g_last_error);
    e->prompt.assign(kept.begin(), kept.begin() + k);
    if (k > 0) e->prompt_used = true;
  });
}
int ohw_engine_set_initial_prompt(ohw_engine* e, const char* text) {
  if (!e) return OHW_E_INVALID_ARG;
  if (!text || !*text) return ohw_engine_set_initial_prompt_tokens(e, nullptr, 0);
  std::vector<int32_t> toks(std::strlen(text) + 1);       // at most one token per byte
  const int n = ohw_tokenize(e->ctx, text, toks.data(), (int)toks.size());
  if (n < 0) return n;
  return ohw_engine_set_initial_prompt_tokens(e, toks.data(), n);
}

int ohw_engine_set_prefill_chunk(ohw_engine* e, int positions) {
  return guard([&] {
    if (!e) throw Error(OHW_E_INVALID_ARG, "engine is null");
    auto set = [&](ohw_state* st) { const int rc = ohw_state_set_prefill_chunk(st, positions); if (rc != OHW_OK) throw Error(rc, g_last_error); };
    set(e->state);
    for (ohw_state* st : e->states) set(st);
    for (ohw_state* st : e->lane_states) set(st);
    e->prefill_chunk = positions;
  });
}

int ohw_engine_set_carry_context(ohw_engine* e, int max_tokens) {
  return guard([&] {
    if (!e) throw Error(OHW_E_INVALID_ARG, "engine is null");
    if (max_tokens < -1) throw Error(OHW_E_INVALID_ARG, "set_carry_context: 0 (off), -1 (the full cap) or a token count, got " + std::to_string(max_tokens));
    e->carry_max = max_tokens;
  });
}

int ohw_engine_last_context(ohw_engine* e, int window, const int32_t** tokens, int* n) {
  return guard([&] {
    if (!e || !tokens || !n) throw Error(OHW_E_INVALID_ARG, "last_context: null argument");
    if (window < 0 || window >= (int)e->last_contexts.size())
      throw Error(OHW_E_INVALID_ARG, "last_context: no window " + std::to_string(window) + " in the last transcribe");
    *tokens = e->last_contexts[(size_t)window].data();
    *n = (int)e->last_contexts[(size_t)window].size();
  });
}

int ohw_engine_long_batch_context(ohw_engine* e, int rec, int window, const int32_t** tokens, int* n) {
  return guard([&] {
    if (!e || !tokens || !n) throw Error(OHW_E_INVALID_ARG, "long_batch_context: null argument");
    if (rec < 0 || rec >= (int)e->batch_records.size()) throw Error(OHW_E_INVALID_ARG, "long_batch_context: no recording " + std::to_string(rec) + " in the last batch call");
    const ohw_engine::BatchRecord& r = e->batch_records[(size_t)rec];
    if (window < 0 || window >= (int)r.contexts.size())
      throw Error(OHW_E_INVALID_ARG, "long_batch_context: recording " + std::to_string(rec) + " has no window " + std::to_string(window));
    *tokens = r.contexts[(size_t)window].data();
    *n = (int)r.contexts[(size_t)window].size();
  });
}

// host only; the seek loops of engine_transcribe_core call it after every window (include/ohw.h states the rule)
int ohw_carry_step_host(int32_t* history, int* n_history, int n_text_ctx, const int32_t* kept, int n_kept, float kept_temperature,
                        int max_tokens, int32_t* context_out, int* n_context_out) {
  return guard([&] {
    if (!history || !n_history || !n_context_out || n_text_ctx < 2 || n_kept < 0 || (n_kept > 0 && !kept) || max_tokens < -1)
      throw Error(OHW_E_INVALID_ARG, "carry_step_host: bad argument");
    const int half = n_text_ctx / 2;
    if (*n_history < 0 || *n_history > half) throw Error(OHW_E_INVALID_ARG, "carry_step_host: the history holds 0 .. n_text_ctx / 2 tokens");
    // a pass kept at T >= 0.5 ran without [prev]: the history starts again from this window alone
    std::vector<int32_t> h;
    if (kept_temperature < 0.5f) h.assign(history, history + *n_history);
    if (n_kept > 0) h.insert(h.end(), kept, kept + n_kept);
    const size_t drop = h.size() > (size_t)half ? h.size() - (size_t)half : 0;
    std::copy(h.begin() + (long)drop, h.end(), history);
    *n_history = (int)(h.size() - drop);
    *n_context_out = 0;
    if (max_tokens == 0 || *n_history == 0) return;
    if (!context_out) throw Error(OHW_E_INVALID_ARG, "carry_step_host: context_out is null");
    std::vector<int32_t> tail((size_t)*n_history);
    const int k = ohw_prompt_clip_host(history, *n_history, n_text_ctx, tail.data());
    if (k < 0) throw Error(OHW_E_INVALID_ARG, "carry_step_host: " + g_last_error);
    const int take = max_tokens > 0 ? std::min(max_tokens, k) : k;
    std::copy(tail.begin() + (k - take), tail.begin() + k, context_out);
    *n_context_out = take;
  });
}

int ohw_engine_set_packed_encoder(ohw_engine* e, int on) {
  if (!e) return OHW_E_INVALID_ARG;
  e->packed_encoder = on != 0;
  (void)ohw_state_set_packed_encoder(e->state, on);
  for (ohw_state* st : e->states) (void)ohw_state_set_packed_encoder(st, on);
  for (ohw_state* st : e->lane_states) (void)ohw_state_set_packed_encoder(st, on);
  return OHW_OK;
}

int ohw_engine_set_force_len(ohw_engine* e, int n_tokens) {
  if (!e || n_tokens < 0) return OHW_E_INVALID_ARG;
  if (n_tokens > 0 && e->beam_size > 0) {       // ohw_beam_search refuses force_len: the setter that comes second fails
    g_last_error = "set_force_len: a beam size is set, and beam search refuses force_len";
    return OHW_E_INVALID_ARG;
  }
  e->force_len = n_tokens;
  return OHW_OK;
}

int ohw_engine_set_beam_size(ohw_engine* e, int k) {
  return guard([&] {
    if (!e) throw Error(OHW_E_INVALID_ARG, "engine is null");
    if (k != 0 && (k < 2 || k > 5)) throw Error(OHW_E_INVALID_ARG, "set_beam_size: 0 (off) or 2..5, got " + std::to_string(k));
    if (k > e->max_batch) throw Error(OHW_E_INVALID_ARG, "set_beam_size: " + std::to_string(k) + " beams need max_batch >= " + std::to_string(k) + ", the engine has " + std::to_string(e->max_batch));
    if (k > 0 && e->force_len > 0) throw Error(OHW_E_INVALID_ARG, "set_beam_size: force_len is set, and beam search refuses it");
    e->beam_size = k;
  });
}

int ohw_engine_set_window_mode(ohw_engine* e, int mode) {
  if (!e || (mode != OHW_WINDOW_FIXED && mode != OHW_WINDOW_SEEK && mode != OHW_WINDOW_FIXED_RECORDING_MEL)) return OHW_E_INVALID_ARG;
  e->window_mode = mode;
  return OHW_OK;
}

int ohw_engine_last_tokens(ohw_engine* e, const int32_t** tokens, int* n) {
  if (!e || !tokens || !n) return OHW_E_INVALID_ARG;
  *tokens = e->last_tokens.data();
  *n = (int)e->last_tokens.size();
  return OHW_OK;
}

int ohw_engine_benchmark(ohw_engine* e, float safety_margin, float* overhead_secs, float* recommended, float* test_audio_secs) {
  return guard([&] {
    if (!e) throw Error(OHW_E_INVALID_ARG, "engine is null");
    const float test_duration = 2.0f;                                         // reference :341
    std::vector<float> silence((size_t)(test_duration * 16000.0f), 0.0f);
    char buf[8];
    (void)ohw_engine_transcribe(e, silence.data(), (int64_t)silence.size(), 16000, buf, sizeof buf, nullptr, nullptr, nullptr);  // warm-up :353
    uint64_t total_ms = 0;
    for (int i = 0; i < 3; ++i) {                                            // :356-365
      const auto t0 = std::chrono::steady_clock::now();
      (void)ohw_engine_transcribe(e, silence.data(), (int64_t)silence.size(), 16000, buf, sizeof buf, nullptr, nullptr, nullptr);
      total_ms += (uint64_t)std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count();
    }
    uint64_t avg_ms = total_ms / 3;                                          // integer average, :367
    // DEVIATION (documented in INTEGRATION.md): the reference has no lower bound, and an engine this
    // fast would round to 0 ms, which silently disables streaming chunks (src/daemon.rs:1189-1193).
    if (avg_ms < 1) avg_ms = 1;
    const float overhead = (float)avg_ms / 1000.0f;                          // :368
    if (overhead_secs) *overhead_secs = overhead;
    if (recommended) *recommended = overhead * (1.0f + safety_margin);       // :373
    if (test_audio_secs) *test_audio_secs = test_duration;
  });
}

}  // extern "C"
