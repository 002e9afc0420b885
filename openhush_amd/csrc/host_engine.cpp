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
// This file: the C ABI entries, validation, samplers, language tables and setters.  What runs behind the transcribe entries
// (windows, decode policy, text assembly) is transcribe.cpp; whisper.cpp's per-window rules are window_policy.cpp.
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

#include "host_engine.hpp"
#include "model.hpp"
#include "window_policy.hpp"

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

template <typename S>
static void trim_spans_of(std::vector<S>& v, size_t lead, size_t new_len) {
  for (S& s : v) {
    size_t o0 = std::max(s.text_off, lead) - lead, o1 = std::max(s.text_off + s.text_len, lead) - lead;
    o0 = std::min(o0, new_len); o1 = std::min(o1, new_len);
    s.text_off = o0; s.text_len = o1 - o0;
  }
}
void trim_spans(std::vector<ohw_span_time>& v, size_t lead, size_t new_len) { trim_spans_of(v, lead, new_len); }
void trim_spans(std::vector<ohw_word_prob>& v, size_t lead, size_t new_len) { trim_spans_of(v, lead, new_len); }

void validate_or_throw(const float* samples, int64_t n, uint32_t sample_rate, ohw_audio_info* info_out, int rec) {
  static const char* const names[] = {"ok", "Audio is empty (no samples)", "Unexpected sample rate", "Audio too long", "Audio too short",
                                      "Audio contains NaN values", "Audio contains infinite values"};
  ohw_audio_info info;
  const int vrc = ohw_validate_audio(samples, n, sample_rate, &info);   // reference :206
  if (info_out) *info_out = info;
  if (vrc != OHW_OK)
    throw Error(OHW_E_VALIDATION, "Audio validation failed" + (rec < 0 ? std::string() : " for recording " + std::to_string(rec)) + ": " + names[info.error]);
}

void check_recording_langs(const char* what, const int32_t* langs, int n_recs, int n_langs) {
  for (int i = 0; langs && i < n_recs; ++i)
    if (langs[i] != OHW_LANG_DETECT && (langs[i] < 0 || langs[i] >= n_langs))
      throw Error(OHW_E_INVALID_ARG, std::string(what) + ": recording " + std::to_string(i) + " asks for language id " + std::to_string(langs[i]));
}

void copy_text_out(char* buf, size_t cap, const std::string& text) {
  if (!buf || cap == 0) return;
  const size_t ncopy = std::min(text.size(), cap - 1);
  std::memcpy(buf, text.data(), ncopy);
  buf[ncopy] = 0;
}

void write_language_out(char* out, const std::string& configured, int32_t id) {
  if (!out) return;
  const std::string lang = configured == "auto" ? ohw_lang_id_to_code(id) : configured;
  std::strncpy(out, lang.c_str(), 7);
  out[7] = 0;
}

int engine_call_ctx(const ohw_engine* e, int64_t n) {
  return e->audio_ctx > 0 ? e->audio_ctx : (e->audio_ctx < 0 && n <= CHUNK_SAMPLES) ? std::min<int>(ohw_audio_ctx_for(n), e->ctx->hp.n_audio_ctx) : 0;
}

void engine_free_overlap(ohw_engine* e) {
  for (size_t i = 1; i < e->states.size(); ++i) ohw_state_free(e->states[i]);
  e->states.clear();
  for (ohw_state* st : e->lane_states) ohw_state_free(st);
  e->lane_states.clear();
  for (void* ls : e->lane_streams) (void)ohw_stream_destroy(ls);
  e->lane_streams.clear();
  for (void** st : {&e->s_full, &e->s_enc, &e->s_dec}) if (*st) { (void)ohw_stream_destroy(*st); *st = nullptr; }
}

bool engine_detects(const ohw_engine* e) { return e->detect_language && e->language == "auto" && e->ctx->hp.n_vocab >= 51865; }

int32_t engine_detect_first_window(ohw_engine* e, const float* samples, int64_t n, float* prob) {
  auto check = [&](int rc) { if (rc != OHW_OK) throw Error(OHW_E_TRANSCRIBE, "Language detection failed: " + g_last_error); };
  if (prob) *prob = 0.f;
  if (mel_frames(n) < 100) return 0;          // less than 1 s: the call yields nothing, whatever the language
  ohw_state* st = e->state;
  check(ohw_state_set_stream(st, nullptr));
  check(ohw_state_set_audio_ctx(st, engine_call_ctx(e, n)));
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
  engine_free_overlap(e);
  ohw_ctx_free(e->ctx);
  delete e;
}

ohw_state* ohw_engine_state(ohw_engine* e) { return e ? e->state : nullptr; }
ohw_ctx* ohw_engine_ctx(ohw_engine* e) { return e ? e->ctx : nullptr; }

int ohw_engine_transcribe(ohw_engine* e, const float* samples, int64_t n, uint32_t sample_rate, char* text_buf, size_t text_cap,
                          char* language_out, uint64_t* duration_ms, ohw_audio_info* info_out) {
  return guard([&] {
    if (!e) throw Error(OHW_E_INVALID_ARG, "engine is null");
    validate_or_throw(samples, n, sample_rate, info_out);
    const auto t0 = std::chrono::steady_clock::now();                       // reference :231
    engine_transcribe(e, samples, n);
    e->last.trim();
    e->last_text = e->last.text;
    copy_text_out(text_buf, text_cap, e->last_text);
    write_language_out(language_out, e->language, e->last_lang_id);
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

int ohw_engine_last_token_times(ohw_engine* e, const ohw_token_time** t, int* n) {
  if (!e || !t || !n) return OHW_E_INVALID_ARG;
  *t = e->last.token_times.data(); *n = (int)e->last.token_times.size();
  return OHW_OK;
}
int ohw_engine_last_words(ohw_engine* e, const ohw_span_time** w, int* n) {
  if (!e || !w || !n) return OHW_E_INVALID_ARG;
  *w = e->last.words.data(); *n = (int)e->last.words.size();
  return OHW_OK;
}
int ohw_engine_last_segments(ohw_engine* e, const ohw_span_time** s, int* n) {
  if (!e || !s || !n) return OHW_E_INVALID_ARG;
  *s = e->last.segments.data(); *n = (int)e->last.segments.size();
  return OHW_OK;
}
int ohw_engine_batch_times(ohw_engine* e, int i, const ohw_token_time** token_times, int* n_token_times, const ohw_span_time** words, int* n_words,
                           const ohw_span_time** segments, int* n_segments) {
  return guard([&] {
    if (!e) throw Error(OHW_E_INVALID_ARG, "engine is null");
    if (i < 0 || i >= (int)e->batch_records.size()) throw Error(OHW_E_INVALID_ARG, "batch_times: no recording " + std::to_string(i) + " in the last transcribe_batch");
    const Transcript& t = e->batch_records[(size_t)i].t;
    if (token_times) *token_times = t.token_times.data();
    if (words) *words = t.words.data();
    if (segments) *segments = t.segments.data();
    if (n_token_times) *n_token_times = (int)t.token_times.size();
    if (n_words) *n_words = (int)t.words.size();
    if (n_segments) *n_segments = (int)t.segments.size();
  });
}

int ohw_engine_set_confidence(ohw_engine* e, int on) {
  return guard([&] {
    if (!e) throw Error(OHW_E_INVALID_ARG, "engine is null");
    e->confidence = on != 0;
    // off: every state of the engine that may have scored gives its buffers back; on: a state allocates when it first scores
    if (!e->confidence) {
      (void)ohw_state_set_score_buffers(e->state, 0);
      for (ohw_state* st : e->states) if (st != e->state) (void)ohw_state_set_score_buffers(st, 0);
      for (ohw_state* st : e->lane_states) (void)ohw_state_set_score_buffers(st, 0);
    }
  });
}
int ohw_engine_last_token_probs(ohw_engine* e, const ohw_token_prob** t, int* n) {
  if (!e || !t || !n) return OHW_E_INVALID_ARG;
  *t = e->last.token_probs.data(); *n = (int)e->last.token_probs.size();
  return OHW_OK;
}
int ohw_engine_last_word_probs(ohw_engine* e, const ohw_word_prob** w, int* n) {
  if (!e || !w || !n) return OHW_E_INVALID_ARG;
  *w = e->last.word_probs.data(); *n = (int)e->last.word_probs.size();
  return OHW_OK;
}
int ohw_engine_last_segment_info(ohw_engine* e, const ohw_segment_info** s, int* n) {
  if (!e || !s || !n) return OHW_E_INVALID_ARG;
  *s = e->last.segment_info.data(); *n = (int)e->last.segment_info.size();
  return OHW_OK;
}
int ohw_engine_batch_confidence(ohw_engine* e, int i, const ohw_token_prob** token_probs, int* n_token_probs, const ohw_word_prob** word_probs,
                                int* n_word_probs, const ohw_segment_info** segment_info, int* n_segments) {
  return guard([&] {
    if (!e) throw Error(OHW_E_INVALID_ARG, "engine is null");
    if (i < 0 || i >= (int)e->batch_records.size()) throw Error(OHW_E_INVALID_ARG, "batch_confidence: no recording " + std::to_string(i) + " in the last batch call");
    const Transcript& t = e->batch_records[(size_t)i].t;
    if (token_probs) *token_probs = t.token_probs.data();
    if (word_probs) *word_probs = t.word_probs.data();
    if (segment_info) *segment_info = t.segment_info.data();
    if (n_token_probs) *n_token_probs = (int)t.token_probs.size();
    if (n_word_probs) *n_word_probs = (int)t.word_probs.size();
    if (n_segments) *n_segments = (int)t.segment_info.size();
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
    for (int i = 0; i < n_recs; ++i) validate_or_throw(recs[i].samples, recs[i].n, sample_rate, nullptr, i);
    engine_transcribe_batch(e, recs, n_recs, lang_ids);
  });
}

int ohw_engine_score_batch(ohw_engine* e, const ohw_audio_span* recs, int n_recs, const int32_t* tokens, const int32_t* offsets, ohw_score_result* results) {
  return guard([&] {
    if (!e || !recs || n_recs < 1 || !tokens || !offsets || !results) throw Error(OHW_E_INVALID_ARG, "score_batch: null argument or no recordings");
    if (e->window_mode != OHW_WINDOW_FIXED) throw Error(OHW_E_INVALID_ARG, "score_batch: recordings are cut as OHW_WINDOW_FIXED cuts; set that window mode");
    for (int i = 0; i < n_recs; ++i) validate_or_throw(recs[i].samples, recs[i].n, 16000, nullptr, i);
    engine_score_batch(e, recs, n_recs, tokens, offsets, results);
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
      validate_or_throw(recs[i].samples, recs[i].n, sample_rate, nullptr, i);
      if (recs[i].n > (int64_t)7200 * 16000)
        throw Error(OHW_E_INVALID_ARG, "transcribe_long_batch: recording " + std::to_string(i) + " is longer than two hours, the limit of a recording slot");
    }
    // the seek loop whatever ohw_engine_set_window_mode says: the per-window bookkeeping reads the mode
    struct Mode { ohw_engine* e; int was; ~Mode() { e->window_mode = was; } } mode{e, e->window_mode};
    e->window_mode = OHW_WINDOW_SEEK;
    engine_transcribe_long_batch(e, recs, n_recs, lang_ids);
  });
}

int ohw_engine_long_batch_quality(ohw_engine* e, int i, const ohw_window_quality** q, int* n_windows) {
  return guard([&] {
    if (!e || !q || !n_windows) throw Error(OHW_E_INVALID_ARG, "long_batch_quality: null argument");
    if (i < 0 || i >= (int)e->batch_records.size()) throw Error(OHW_E_INVALID_ARG, "long_batch_quality: no recording " + std::to_string(i) + " in the last batch call");
    const ohw_engine::BatchRecord& r = e->batch_records[(size_t)i];
    *q = r.t.quality.data();
    *n_windows = (int)r.n_windows();
  });
}

// ---- speech-aware windows (include/ohw.h) ------------------------------------------------------------------------------------
int ohw_engine_set_vad(ohw_engine* e, const ohw_vad_config* cfg, const ohw_vad_detector* det, const ohw_chunk_plan* plan) {
  return guard([&] {
    if (!e) throw Error(OHW_E_INVALID_ARG, "engine is null");
    ohw_vad_config c; ohw_vad_detector d; ohw_chunk_plan p;
    if (cfg) c = *cfg; else ohw_default_vad_config(&c);
    if (det) d = *det; else ohw_default_vad_detector(&d);
    if (plan) p = *plan; else ohw_default_chunk_plan(&p);
    if (!std::isfinite(c.threshold)) throw Error(OHW_E_INVALID_ARG, "set_vad: the threshold is not finite");
    if (!std::isfinite(d.floor_quantile) || !std::isfinite(d.margin_db) || !std::isfinite(d.slope_db) || !(d.floor_quantile > 0.0f) ||
        !(d.floor_quantile <= 1.0f) || !(d.slope_db > 0.0f))
      throw Error(OHW_E_INVALID_ARG, "set_vad: floor_quantile must be in (0, 1], slope_db above 0, and all three finite");
    if (!std::isfinite(p.max_chunk_s) || !(p.max_chunk_s > 0.0f) || p.max_chunk_s > 30.0f || (double)p.min_chunk_ms * 16.0 > (double)p.max_chunk_s * 16000.0)
      throw Error(OHW_E_INVALID_ARG, "set_vad: max_chunk_s must be in (0, 30] and cover min_chunk_ms");
    e->vad_cfg = c; e->vad_det = d; e->chunk_plan = p;
  });
}

int ohw_engine_transcribe_speech(ohw_engine* e, const ohw_audio_span* recs, const ohw_frame_probs* probs, int n_recs, uint32_t sample_rate) {
  return ohw_engine_transcribe_speech_lang(e, recs, probs, nullptr, n_recs, sample_rate);
}

int ohw_engine_transcribe_speech_lang(ohw_engine* e, const ohw_audio_span* recs, const ohw_frame_probs* probs, const int32_t* lang_ids,
                                      int n_recs, uint32_t sample_rate) {
  return guard([&] {
    if (!e || !recs || n_recs < 1) throw Error(OHW_E_INVALID_ARG, "transcribe_speech: null engine or no recordings");
    if (e->window_mode != OHW_WINDOW_FIXED) throw Error(OHW_E_INVALID_ARG, "transcribe_speech: chunks are cut as OHW_WINDOW_FIXED cuts; set that window mode");
    e->batch_records.clear();
    for (int i = 0; i < n_recs; ++i) validate_or_throw(recs[i].samples, recs[i].n, sample_rate, nullptr, i);
    engine_transcribe_speech(e, recs, probs, n_recs, lang_ids);
  });
}

int ohw_engine_speech_chunks(ohw_engine* e, int i, const ohw_speech_chunk** chunks, int* n, const ohw_window_quality** quality) {
  return guard([&] {
    if (!e) throw Error(OHW_E_INVALID_ARG, "engine is null");
    if (i < 0 || i >= (int)e->batch_records.size()) throw Error(OHW_E_INVALID_ARG, "speech_chunks: no recording " + std::to_string(i) + " in the last batch call");
    const ohw_engine::BatchRecord& r = e->batch_records[(size_t)i];
    if (chunks) *chunks = r.chunks.data();
    if (n) *n = (int)r.chunks.size();
    if (quality) *quality = r.t.quality.data();
  });
}

int ohw_engine_speech_segments(ohw_engine* e, int i, const ohw_speech_segment** segments, int* n) {
  return guard([&] {
    if (!e) throw Error(OHW_E_INVALID_ARG, "engine is null");
    if (i < 0 || i >= (int)e->batch_records.size()) throw Error(OHW_E_INVALID_ARG, "speech_segments: no recording " + std::to_string(i) + " in the last batch call");
    const ohw_engine::BatchRecord& r = e->batch_records[(size_t)i];
    if (segments) *segments = r.speech.data();
    if (n) *n = (int)r.speech.size();
  });
}

int ohw_engine_batch_result(ohw_engine* e, int i, const char** text, size_t* text_len, const int32_t** tokens, int* n_tokens,
                            const ohw_window_quality** quality, char* language_out) {
  return guard([&] {
    if (!e) throw Error(OHW_E_INVALID_ARG, "engine is null");
    if (i < 0 || i >= (int)e->batch_records.size()) throw Error(OHW_E_INVALID_ARG, "batch_result: no recording " + std::to_string(i) + " in the last transcribe_batch");
    const ohw_engine::BatchRecord& r = e->batch_records[(size_t)i];
    if (text) *text = r.t.text.c_str();
    if (text_len) *text_len = r.t.text.size();
    if (tokens) *tokens = r.t.tokens.data();
    if (n_tokens) *n_tokens = (int)r.t.tokens.size();
    if (quality) *quality = r.t.quality.empty() ? &r.none : r.t.quality.data();     // long batch: one record per window
    // a recording decoded in a language of its own reports that one, whatever the engine is configured with
    write_language_out(language_out, r.lang_id >= 0 ? std::string("auto") : e->language, std::max(r.lang_id, 0));
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
  *q = e->last.quality.data();
  *n_windows = (int)e->last.quality.size();
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

int ohw_engine_set_hot_phrases_tokens(ohw_engine* e, const int32_t* tokens, const int32_t* offsets, const float* boosts, int n_phrases) {
  return guard([&] {
    if (!e || n_phrases < 0 || (n_phrases > 0 && (!tokens || !offsets))) throw Error(OHW_E_INVALID_ARG, "hot phrases: bad argument");
    const std::vector<float> ones((size_t)n_phrases, 1.0f);
    if (!boosts) boosts = ones.data();
    // on the engine's own state: the next transcribe hands its rules to the other states it decodes on (transcribe.cpp)
    const int rc = ohw_state_set_phrase_table(e->state, tokens, offsets, boosts, n_phrases);
    if (rc != OHW_OK) throw Error(rc, g_last_error);
  });
}
int ohw_engine_set_hot_phrases(ohw_engine* e, const char* const* texts, const float* boosts, int n) {
  if (!e || n < 0 || (n > 0 && !texts)) return OHW_E_INVALID_ARG;
  // every phrase in two variants, duplicates dropped: " text" (mid-sentence) and "text" (window start)
  std::vector<int32_t> toks, offs{0};
  std::vector<float> bs;
  std::vector<std::vector<int32_t>> seen;
  for (int i = 0; i < n; ++i) {
    if (!texts[i]) return OHW_E_INVALID_ARG;
    const std::string given = texts[i];
    bool any = false;
    for (const std::string& form : {" " + given, given}) {
      std::vector<int32_t> t(form.size() + 1);       // at most one token per byte
      const int k = ohw_tokenize(e->ctx, form.c_str(), t.data(), (int)t.size());
      if (k < 0) return k;
      if (k == 0) continue;                          // nothing of this form is in the vocabulary
      any = true;
      t.resize((size_t)k);
      if (std::find(seen.begin(), seen.end(), t) != seen.end()) continue;
      seen.push_back(t);
      toks.insert(toks.end(), t.begin(), t.end());
      offs.push_back((int32_t)toks.size());
      bs.push_back(boosts ? boosts[i] : 1.0f);
    }
    if (!any) {
      g_last_error = "hot phrases: text " + std::to_string(i) + " has no token in this vocabulary";
      return OHW_E_INVALID_ARG;
    }
  }
  return ohw_engine_set_hot_phrases_tokens(e, toks.data(), offs.data(), bs.data(), (int)bs.size());
}

int ohw_engine_set_repetition(ohw_engine* e, float penalty, int ngram) {
  return guard([&] {
    // on the engine's own state, as above (the state setter checks the values ahead of the state)
    const int rc = ohw_state_set_repeat_rule(e ? e->state : nullptr, penalty, ngram);
    if (rc != OHW_OK) throw Error(rc, g_last_error);
  });
}

static void engine_set_commands_tokens(ohw_engine* e, const int32_t* tokens, const int32_t* offsets, int n_phrases, float penalty, std::vector<int32_t> index) {
  if (!e || n_phrases < 0 || (n_phrases > 0 && (!tokens || !offsets))) throw Error(OHW_E_INVALID_ARG, "commands: bad argument");
  // on the engine's own state, as the hot phrases
  const int rc = ohw_state_set_command_table(e->state, tokens, offsets, n_phrases, penalty);
  if (rc != OHW_OK) throw Error(rc, g_last_error);
  e->cmd_index.swap(index);
}

int ohw_engine_set_commands_tokens(ohw_engine* e, const int32_t* tokens, const int32_t* offsets, int n_phrases, float penalty) {
  return guard([&] {
    std::vector<int32_t> index((size_t)std::max(0, n_phrases));
    for (size_t i = 0; i < index.size(); ++i) index[i] = (int32_t)i;
    engine_set_commands_tokens(e, tokens, offsets, n_phrases, penalty, std::move(index));
  });
}

int ohw_engine_set_commands(ohw_engine* e, const char* const* texts, int n, float penalty) {
  return guard([&] {
    if (!e || n < 0 || (n > 0 && !texts)) throw Error(OHW_E_INVALID_ARG, "commands: bad argument");
    // every text in up to two forms under the text's index: "text" (window start) and " text"; a form equal to the other is dropped
    std::vector<int32_t> toks, offs{0}, index;
    for (int i = 0; i < n; ++i) {
      if (!texts[i]) throw Error(OHW_E_INVALID_ARG, "commands: text " + std::to_string(i) + " is null");
      const std::string given = texts[i];
      std::vector<int32_t> first;
      for (const std::string& form : {given, " " + given}) {
        std::vector<int32_t> t(form.size() + 1);       // at most one token per byte
        const int k = ohw_tokenize(e->ctx, form.c_str(), t.data(), (int)t.size());
        if (k < 0) throw Error(k, g_last_error);
        if (k == 0) continue;                          // nothing of this form is in the vocabulary
        t.resize((size_t)k);
        if (t == first) continue;
        if (first.empty()) first = t;
        toks.insert(toks.end(), t.begin(), t.end());
        offs.push_back((int32_t)toks.size());
        index.push_back(i);
      }
      if (first.empty()) throw Error(OHW_E_INVALID_ARG, "commands: text " + std::to_string(i) + " ('" + given + "') has no token in this vocabulary");
    }
    const int n_forms = (int)index.size();
    engine_set_commands_tokens(e, toks.data(), offs.data(), n_forms, penalty, std::move(index));
  });
}

int ohw_engine_last_commands(ohw_engine* e, const ohw_command_hit** hits, int* n) {
  if (!e || !hits || !n) return OHW_E_INVALID_ARG;
  *hits = e->last.commands.data();
  *n = (int)e->last.commands.size();
  return OHW_OK;
}

int ohw_engine_batch_commands(ohw_engine* e, int i, const ohw_command_hit** hits, int* n) {
  return guard([&] {
    if (!e || !hits || !n) throw Error(OHW_E_INVALID_ARG, "batch_commands: null argument");
    if (i < 0 || i >= (int)e->batch_records.size()) throw Error(OHW_E_INVALID_ARG, "batch_commands: no recording " + std::to_string(i) + " in the last batch call");
    *hits = e->batch_records[(size_t)i].t.commands.data();
    *n = (int)e->batch_records[(size_t)i].t.commands.size();
  });
}

int ohw_engine_set_prefill_chunk(ohw_engine* e, int positions) {
  return guard([&] {
    if (!e) throw Error(OHW_E_INVALID_ARG, "engine is null");
    auto set = [&](ohw_state* st) { const int rc = ohw_state_set_prefill_chunk(st, positions); if (rc != OHW_OK) throw Error(rc, g_last_error); };
    each_state(e, set);
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

int ohw_engine_set_stitch(ohw_engine* e, int overlap_ms) {
  return guard([&] {
    if (!e) throw Error(OHW_E_INVALID_ARG, "engine is null");
    const int rc = ohw_stitch_plan_host(0, overlap_ms, nullptr, nullptr);      // the one place that judges an overlap
    if (rc != OHW_OK) throw Error(rc, g_last_error);
    e->stitch_ms = overlap_ms;
  });
}

int ohw_engine_stitch(ohw_engine* e) { return e ? e->stitch_ms : OHW_E_INVALID_ARG; }

int ohw_engine_last_seams(ohw_engine* e, const ohw_seam** seams, int* n) {
  if (!e || !seams || !n) return OHW_E_INVALID_ARG;
  *seams = e->last_seams.data();
  *n = (int)e->last_seams.size();
  return OHW_OK;
}

int ohw_engine_last_window_tokens(ohw_engine* e, const int32_t** tokens, const int32_t** offsets, int* n_windows) {
  if (!e || !tokens || !offsets || !n_windows) return OHW_E_INVALID_ARG;
  *tokens = e->last_win_tokens.data();
  *offsets = e->last_win_offsets.data();
  *n_windows = e->last_win_offsets.empty() ? 0 : (int)e->last_win_offsets.size() - 1;
  return OHW_OK;
}

int ohw_engine_last_context(ohw_engine* e, int window, const int32_t** tokens, int* n) {
  return guard([&] {
    if (!e || !tokens || !n) throw Error(OHW_E_INVALID_ARG, "last_context: null argument");
    if (window < 0 || window >= (int)e->last.contexts.size())
      throw Error(OHW_E_INVALID_ARG, "last_context: no window " + std::to_string(window) + " in the last transcribe");
    *tokens = e->last.contexts[(size_t)window].data();
    *n = (int)e->last.contexts[(size_t)window].size();
  });
}

int ohw_engine_long_batch_context(ohw_engine* e, int rec, int window, const int32_t** tokens, int* n) {
  return guard([&] {
    if (!e || !tokens || !n) throw Error(OHW_E_INVALID_ARG, "long_batch_context: null argument");
    if (rec < 0 || rec >= (int)e->batch_records.size()) throw Error(OHW_E_INVALID_ARG, "long_batch_context: no recording " + std::to_string(rec) + " in the last batch call");
    const ohw_engine::BatchRecord& r = e->batch_records[(size_t)rec];
    if (window < 0 || window >= (int)r.n_windows())
      throw Error(OHW_E_INVALID_ARG, "long_batch_context: recording " + std::to_string(rec) + " has no window " + std::to_string(window));
    *tokens = r.t.contexts[(size_t)window].data();
    *n = (int)r.t.contexts[(size_t)window].size();
  });
}

// host only; the seek loops of transcribe.cpp call it after every window (include/ohw.h states the rule)
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
  each_state(e, [&](ohw_state* st) { (void)ohw_state_set_packed_encoder(st, on); });
  return OHW_OK;
}

int ohw_engine_set_force_len(ohw_engine* e, int n_tokens) {
  if (!e || n_tokens < 0) return OHW_E_INVALID_ARG;
  if (n_tokens > 0 && e->beam_size > 0) {       // ohw_beam_search refuses force_len: the setter that comes second fails
    g_last_error = "set_force_len: a beam size is set, and beam search refuses force_len";
    return OHW_E_INVALID_ARG;
  }
  if (n_tokens > 0 && e->best_of > 1) {
    g_last_error = "set_force_len: best_of is set, and best-of sampling refuses force_len";
    return OHW_E_INVALID_ARG;
  }
  e->force_len = n_tokens;
  return OHW_OK;
}

int ohw_engine_set_best_of(ohw_engine* e, int n) {
  return guard([&] {
    if (!e) throw Error(OHW_E_INVALID_ARG, "engine is null");
    if (n < 1 || n > 5) throw Error(OHW_E_INVALID_ARG, "set_best_of: 1 (off) .. 5, got " + std::to_string(n));
    if (n > e->max_batch) throw Error(OHW_E_INVALID_ARG, "set_best_of: " + std::to_string(n) + " candidates need max_batch >= " + std::to_string(n) + ", the engine has " + std::to_string(e->max_batch));
    if (n > 1 && e->force_len > 0) throw Error(OHW_E_INVALID_ARG, "set_best_of: force_len is set, and best-of sampling refuses it");
    e->best_of = n;
  });
}

int ohw_engine_last_candidates(ohw_engine* e, const int32_t** data, int* n) {
  if (!e || !data || !n) return OHW_E_INVALID_ARG;
  *data = e->last_cands.data();
  *n = (int)e->last_cands.size();
  return OHW_OK;
}

int ohw_engine_last_candidate_logprobs(ohw_engine* e, const float** data, int* n) {
  if (!e || !data || !n) return OHW_E_INVALID_ARG;
  *data = e->last_cand_lps.data();
  *n = (int)e->last_cand_lps.size();
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
  *tokens = e->last.tokens.data();
  *n = (int)e->last.tokens.size();
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
