// vad.cpp — the step in front of the path in continuous mode: voice-activity segmentation, host code.
//
//   ohw_vad_state_*    <- VadState (reference src/vad/mod.rs:112-250): the speech / silence state machine that turns per-chunk
//                         VAD results into speech segments (min_silence_ms to end a segment, min_speech_ms to keep it)
//   ohw_vad_engine     <- trait VadEngine (reference src/vad/mod.rs:34-55): process(samples) -> probability, reset,
//                         chunk_size, sample_rate - as a C struct of function pointers, so the reference's SileroVad (an ONNX
//                         model the reference loads through the silero-vad-rust crate; neither is available offline) or any
//                         other detector plugs in from the host side
//   ohw_vad_run        <- the daemon's continuous-mode loop (reference src/daemon.rs:2062-2138): every poll the audio since
//                         the last poll goes through the engine, the result through the state machine, and a completed
//                         segment is cut from the first speech poll to the current position
//   ohw_vad_energy_engine  a built-in detector for tests and for hosts without a model: short-time RMS against a threshold.
//                         It is NOT Silero and makes no claim to its accuracy.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "common.hpp"

struct ohw_vad_state {
  ohw_vad_config cfg;
  uint32_t sample_rate;
  std::vector<float> probabilities;
  bool in_speech = false;
  bool has_start = false;
  int64_t speech_start = 0;
  int64_t silence_samples = 0;
  int64_t total_samples = 0;
};

extern "C" {

void ohw_default_vad_config(ohw_vad_config* c) {        // reference src/vad/mod.rs:76-100
  if (!c) return;
  c->enabled = 0; c->threshold = 0.5f; c->min_silence_ms = 700; c->min_speech_ms = 250; c->speech_pad_ms = 30;
}

ohw_vad_state* ohw_vad_state_new(const ohw_vad_config* cfg, uint32_t sample_rate) {
  ohw_vad_state* s = new (std::nothrow) ohw_vad_state();
  if (!s) return nullptr;
  if (cfg) s->cfg = *cfg; else ohw_default_vad_config(&s->cfg);
  s->sample_rate = sample_rate;
  return s;
}

void ohw_vad_state_free(ohw_vad_state* s) { delete s; }

// VadState::update (reference src/vad/mod.rs:158-224)
int ohw_vad_state_update(ohw_vad_state* s, float probability, int is_speech, int64_t chunk_samples, ohw_speech_segment* seg) {
  if (!s || chunk_samples < 0) return OHW_E_INVALID_ARG;
  s->probabilities.push_back(probability);
  const int64_t prev_total = s->total_samples;
  s->total_samples += chunk_samples;
  const int64_t min_silence = (int64_t)((float)s->cfg.min_silence_ms / 1000.0f * (float)s->sample_rate);
  const int64_t min_speech = (int64_t)((float)s->cfg.min_speech_ms / 1000.0f * (float)s->sample_rate);
  if (is_speech) {
    s->silence_samples = 0;
    if (!s->in_speech) {                       // speech just started
      s->in_speech = true;
      s->has_start = true;
      s->speech_start = prev_total;
    }
    return 0;
  }
  s->silence_samples += chunk_samples;
  if (s->in_speech && s->silence_samples >= min_silence) {   // speech ended
    s->in_speech = false;
    const int64_t start = s->has_start ? s->speech_start : 0;
    s->has_start = false;
    const int64_t end = prev_total;            // the segment ends where this chunk of silence starts
    if (end - start >= min_speech) {
      float avg = 0.0f;
      if (!s->probabilities.empty()) {
        float sum = 0.0f;
        for (float p : s->probabilities) sum += p;
        avg = sum / (float)s->probabilities.size();
      }
      s->probabilities.clear();
      if (seg) { seg->start = start; seg->end = end; seg->avg_probability = avg; }
      return 1;
    }
    s->probabilities.clear();                  // too short: dropped
  }
  return 0;
}

int ohw_vad_state_is_speech(const ohw_vad_state* s) { return s && s->in_speech ? 1 : 0; }
int64_t ohw_vad_state_speech_start(const ohw_vad_state* s) { return s && s->has_start ? s->speech_start : -1; }
void ohw_vad_state_reset(ohw_vad_state* s) {
  if (!s) return;
  s->probabilities.clear();
  s->in_speech = false; s->has_start = false; s->speech_start = 0; s->silence_samples = 0; s->total_samples = 0;
}

// ---- built-in energy detector (a VadEngine implementation; not Silero) -------------------------------------------------
namespace {
struct EnergyVad { float threshold_db; };
int energy_process(void* user, const float* samples, int64_t n, float* probability) {
  const EnergyVad* v = (const EnergyVad*)user;
  if (n <= 0) { *probability = 0.0f; return 0; }
  // like SileroVad::process the result is the mean over 512-sample chunks (reference src/vad/silero.rs:39-94); the score
  // of a chunk is a logistic of its level in dB around the threshold (6 dB per unit)
  double total = 0.0;
  int64_t count = 0;
  for (int64_t off = 0; off < n; off += 512) {
    const int64_t len = n - off < 512 ? n - off : 512;
    double ss = 0.0;
    for (int64_t i = 0; i < len; ++i) ss += (double)samples[off + i] * samples[off + i];
    const double rms = std::sqrt(ss / 512.0);                       // a partial chunk is zero-padded to 512, as the reference pads
    const double db = rms > 1e-10 ? 20.0 * std::log10(rms) : -200.0;
    total += 1.0 / (1.0 + std::exp(-(db - (double)v->threshold_db) / 6.0));
    ++count;
  }
  *probability = (float)(total / (double)count);
  return 0;
}
void energy_reset(void*) {}
}  // namespace

int ohw_vad_energy_engine(float threshold_db, ohw_vad_engine* out) {
  if (!out) return OHW_E_INVALID_ARG;
  EnergyVad* v = new (std::nothrow) EnergyVad{threshold_db};
  if (!v) return OHW_E_OOM;
  out->user = v; out->process = energy_process; out->reset = energy_reset; out->chunk_size = 512; out->sample_rate = 16000;
  return OHW_OK;
}
void ohw_vad_energy_engine_free(ohw_vad_engine* e) {
  if (e && e->process == energy_process) { delete (EnergyVad*)e->user; e->user = nullptr; }
}

// The daemon's continuous-mode loop over a whole recording (reference src/daemon.rs:2062-2138): polls of poll_samples; the
// audio since the last poll is one engine.process call (is_speech = probability >= threshold); the first speech poll marks
// the segment start; when the state machine completes a segment it is cut at the CURRENT position (the reference extracts
// [speech_start_pos, current_pos), i.e. the trailing min_silence stays inside the cut).  Returns the number of segments
// (all of them; at most cap are written), or a negative error code.
int64_t ohw_vad_run(const ohw_vad_engine* engine, const ohw_vad_config* cfg, const float* samples, int64_t n, int64_t poll_samples,
                    ohw_speech_segment* out, int64_t cap) {
  if (!engine || !engine->process || !cfg || (!samples && n > 0) || poll_samples <= 0) return OHW_E_INVALID_ARG;
  ohw_vad_state* st = ohw_vad_state_new(cfg, engine->sample_rate);
  if (!st) return OHW_E_OOM;
  if (engine->reset) engine->reset(engine->user);
  int64_t n_seg = 0, last = 0, speech_start_pos = -1;
  while (last < n) {
    const int64_t cur = last + poll_samples < n ? last + poll_samples : n;
    float prob = 0.0f;
    if (engine->process(engine->user, samples + last, cur - last, &prob) != 0) { ohw_vad_state_free(st); return OHW_E_TRANSCRIBE; }
    const int is_speech = prob >= cfg->threshold ? 1 : 0;
    if (is_speech && speech_start_pos < 0) speech_start_pos = last;
    ohw_speech_segment seg{};
    if (ohw_vad_state_update(st, prob, is_speech, cur - last, &seg) == 1) {
      const int64_t start = speech_start_pos >= 0 ? speech_start_pos : seg.start;
      speech_start_pos = -1;
      if (n_seg < cap && out) { out[n_seg].start = start; out[n_seg].end = cur; out[n_seg].avg_probability = seg.avg_probability; }
      ++n_seg;
    }
    last = cur;
  }
  ohw_vad_state_free(st);
  return n_seg;
}

// ---- speech-aware windows: the plan (include/ohw.h).  This project's own rules, host only; tests/vad_ref.py restates them ------
void ohw_default_chunk_plan(ohw_chunk_plan* p) {
  if (!p) return;
  p->max_chunk_s = 30.0f; p->max_gap_ms = 2000; p->min_chunk_ms = 1100;
}

int64_t ohw_speech_segments_host(const float* probs, int64_t n_probs, int frame_samples, int64_t n_samples, const ohw_vad_config* cfg,
                                 ohw_speech_segment* out, int64_t cap) {
  if (n_probs < 0 || (!probs && n_probs > 0) || frame_samples < 1 || n_samples < 0 || cap < 0 || (!out && cap > 0)) return OHW_E_INVALID_ARG;
  ohw_vad_config c;
  if (cfg) c = *cfg; else ohw_default_vad_config(&c);
  if (!std::isfinite(c.threshold)) return OHW_E_INVALID_ARG;
  const float thr = c.threshold, neg = std::max(thr - 0.15f, 0.01f);
  const int64_t fs = frame_samples, min_silence = (int64_t)c.min_silence_ms * 16, min_speech = (int64_t)c.min_speech_ms * 16, pad = (int64_t)c.speech_pad_ms * 16;
  struct Raw { int64_t f0, f1; };
  std::vector<Raw> raw;
  bool open = false;
  int64_t start = 0, pending = -1;
  for (int64_t f = 0; f < n_probs; ++f) {
    const float p = probs[f];
    if (p >= thr) {
      if (!open) { open = true; start = f; }
      pending = -1;
    } else if (open) {
      if (p < neg && pending < 0) pending = f;
      if (pending >= 0 && (f + 1 - pending) * fs >= min_silence) {
        if ((pending - start) * fs >= min_speech) raw.push_back(Raw{start, pending});
        open = false; pending = -1;
      }
    }
  }
  if (open && (n_probs - start) * fs >= min_speech) raw.push_back(Raw{start, n_probs});
  const int64_t n_seg = (int64_t)raw.size();
  // pads: both sides; neighbours whose pads would meet share the gap at its midpoint; clipped to the recording
  std::vector<int64_t> s((size_t)n_seg), e((size_t)n_seg);
  for (int64_t i = 0; i < n_seg; ++i) { s[(size_t)i] = raw[(size_t)i].f0 * fs; e[(size_t)i] = raw[(size_t)i].f1 * fs; }
  for (int64_t i = 0; i < n_seg; ++i) {
    int64_t a = s[(size_t)i] - pad, b = e[(size_t)i] + pad;
    if (i > 0) {
      const int64_t gap = s[(size_t)i] - e[(size_t)i - 1];
      if (gap < 2 * pad) a = e[(size_t)i - 1] + gap / 2;
    }
    if (i + 1 < n_seg) {
      const int64_t gap = s[(size_t)i + 1] - e[(size_t)i];
      if (gap < 2 * pad) b = e[(size_t)i] + gap / 2;
    }
    a = std::min(std::max<int64_t>(a, 0), n_samples);
    b = std::min(std::max<int64_t>(b, 0), n_samples);
    if (i < cap) {
      double sum = 0.0;
      for (int64_t f = raw[(size_t)i].f0; f < raw[(size_t)i].f1; ++f) sum += (double)probs[f];
      out[i].start = a; out[i].end = b;
      out[i].avg_probability = (float)(sum / (double)(raw[(size_t)i].f1 - raw[(size_t)i].f0));
    }
  }
  return n_seg;
}

int64_t ohw_speech_chunks_host(const ohw_speech_segment* segments, int64_t n_seg, const float* probs, int64_t n_probs, int frame_samples,
                               int64_t n_samples, const ohw_chunk_plan* plan, ohw_speech_chunk* out, int64_t cap) {
  if (n_seg < 0 || (!segments && n_seg > 0) || n_probs < 0 || (!probs && n_probs > 0) || frame_samples < 1 || n_samples < 0 || cap < 0 ||
      (!out && cap > 0))
    return OHW_E_INVALID_ARG;
  ohw_chunk_plan pl;
  if (plan) pl = *plan; else ohw_default_chunk_plan(&pl);
  if (!std::isfinite(pl.max_chunk_s) || !(pl.max_chunk_s > 0.0f) || pl.max_chunk_s > 30.0f) return OHW_E_INVALID_ARG;
  const int64_t fs = frame_samples, max_len = (int64_t)((double)pl.max_chunk_s * 16000.0), max_gap = (int64_t)pl.max_gap_ms * 16,
                min_chunk = (int64_t)pl.min_chunk_ms * 16;
  if (max_len < 2 || min_chunk > max_len) return OHW_E_INVALID_ARG;
  for (int64_t i = 0; i < n_seg; ++i)
    if (segments[i].start < 0 || segments[i].end < segments[i].start || segments[i].end > n_samples || (i > 0 && segments[i].start < segments[i - 1].end))
      return OHW_E_INVALID_ARG;
  std::vector<ohw_speech_chunk> ch;
  bool have = false;
  ohw_speech_chunk cur{};
  int64_t prev_end = 0;
  for (int64_t i = 0; i < n_seg; ++i) {
    int64_t s = segments[i].start;
    const int64_t e = segments[i].end;
    if (have && (s - prev_end > max_gap || e - cur.start > max_len)) { ch.push_back(cur); have = false; }
    if (!have) {
      // a segment longer than a chunk: cut at the frame of lowest p among those that start in [s + max_len / 2, s + max_len)
      while (e - s > max_len) {
        const int64_t lo = s + max_len / 2, hi = s + max_len;
        int64_t cut = hi;
        float best = 0.0f;
        bool found = false;
        for (int64_t f = (lo + fs - 1) / fs; f < n_probs && f * fs < hi; ++f)
          if (!found || probs[f] < best) { best = probs[f]; cut = f * fs; found = true; }
        ch.push_back(ohw_speech_chunk{s, cut, (int32_t)i, 1});
        s = cut;
      }
      cur = ohw_speech_chunk{s, e, (int32_t)i, 1};
      have = true;
    } else {
      cur.end = e;
      ++cur.n_segments;
    }
    prev_end = e;
  }
  if (have) ch.push_back(cur);
  // a short chunk grows evenly on both sides, bounded by its neighbours (the earlier one as already grown) and the recording
  const int64_t n_ch = (int64_t)ch.size();
  for (int64_t c = 0; c < n_ch; ++c) {
    ohw_speech_chunk& k = ch[(size_t)c];
    const int64_t need = min_chunk - (k.end - k.start);
    if (need <= 0) continue;
    const int64_t avail_l = k.start - (c > 0 ? ch[(size_t)c - 1].end : 0), avail_r = (c + 1 < n_ch ? ch[(size_t)c + 1].start : n_samples) - k.end;
    int64_t a = std::min(need / 2, avail_l);
    const int64_t b = std::min(need - a, avail_r);
    a = std::min(need - b, avail_l);
    k.start -= a; k.end += b;
  }
  for (int64_t c = 0; c < n_ch && c < cap; ++c) out[c] = ch[(size_t)c];
  return n_ch;
}

}  // extern "C"
