// A stand-alone host program over ohw_speech_segments_host / ohw_speech_chunks_host (csrc/vad.cpp), meant to be built with
// AddressSanitizer and UBSan on the host side (tests/test_vad_plan_sanitized.py): seeded probability tracks of many shapes, output
// arrays of exactly the reported size or smaller (a write behind `cap` is a heap overflow the sanitizer reports), empty and
// degenerate arguments.  It checks only what needs no second implementation: ordering, bounds, and that a short `cap` changes
// nothing but how much is written.  Prints "plan ok" and the totals.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/ohw.h"

static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static float rndf() { return (float)(rnd() % 10000) / 10000.0f; }

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "vad_plan_main: %s failed at line %d (case %d)\n", #c, __LINE__, g_case); return 1; } } while (0)
static int g_case = 0;

int main() {
  long total_seg = 0, total_ch = 0;
  const int frame_sizes[3] = {160, 512, 1};
  for (g_case = 0; g_case < 400; ++g_case) {
    const int fs = frame_sizes[g_case % 3];
    const int64_t n_probs = g_case < 4 ? g_case : (int64_t)(rnd() % (fs == 1 ? 20000 : 12000)) + 1;
    std::vector<float> p((size_t)n_probs);
    for (int64_t f = 0; f < n_probs;) {
      const int64_t run = (int64_t)(rnd() % 700) + 1;
      const float level = (rnd() % 3) ? 0.8f : 0.05f;
      for (int64_t k = 0; k < run && f < n_probs; ++k, ++f) p[(size_t)f] = level + 0.15f * (rndf() - 0.5f);
    }
    const int64_t n = n_probs * fs - (n_probs > 0 ? (int64_t)(rnd() % (uint32_t)fs) : 0);
    ohw_vad_config cfg;
    ohw_default_vad_config(&cfg);
    cfg.min_silence_ms = (rnd() % 4) * 300; cfg.min_speech_ms = (rnd() % 3) * 200; cfg.speech_pad_ms = (rnd() % 3) * 200;
    ohw_chunk_plan plan;
    ohw_default_chunk_plan(&plan);
    plan.max_chunk_s = (rnd() % 2) ? 30.0f : 4.0f; plan.max_gap_ms = (rnd() % 3) * 1000; plan.min_chunk_ms = (rnd() % 2) ? 1100 : 0;
    const int64_t n_seg = ohw_speech_segments_host(p.data(), n_probs, fs, n, &cfg, nullptr, 0);
    CHECK(n_seg >= 0 && n_seg <= n_probs / 2 + 1);
    std::vector<ohw_speech_segment> seg((size_t)n_seg), few((size_t)(n_seg / 2));
    CHECK(ohw_speech_segments_host(p.data(), n_probs, fs, n, &cfg, seg.data(), n_seg) == n_seg);
    CHECK(ohw_speech_segments_host(p.data(), n_probs, fs, n, &cfg, few.data(), (int64_t)few.size()) == n_seg);
    for (int64_t i = 0; i < n_seg; ++i) {
      CHECK(seg[(size_t)i].start >= 0 && seg[(size_t)i].start <= seg[(size_t)i].end && seg[(size_t)i].end <= n);
      CHECK(i == 0 || seg[(size_t)i].start >= seg[(size_t)i - 1].end);
      CHECK(seg[(size_t)i].avg_probability >= 0.0f && seg[(size_t)i].avg_probability <= 1.0f);
      CHECK((size_t)i >= few.size() || (few[(size_t)i].start == seg[(size_t)i].start && few[(size_t)i].end == seg[(size_t)i].end));
    }
    const int64_t n_ch = ohw_speech_chunks_host(seg.data(), n_seg, p.data(), n_probs, fs, n, &plan, nullptr, 0);
    CHECK(n_ch >= 0);
    std::vector<ohw_speech_chunk> ch((size_t)n_ch), one((size_t)(n_ch > 0 ? 1 : 0));
    CHECK(ohw_speech_chunks_host(seg.data(), n_seg, p.data(), n_probs, fs, n, &plan, ch.data(), n_ch) == n_ch);
    CHECK(ohw_speech_chunks_host(seg.data(), n_seg, p.data(), n_probs, fs, n, &plan, one.data(), (int64_t)one.size()) == n_ch);
    const int64_t max_len = (int64_t)((double)plan.max_chunk_s * 16000.0);
    for (int64_t c = 0; c < n_ch; ++c) {
      const ohw_speech_chunk& k = ch[(size_t)c];
      CHECK(k.start >= 0 && k.start < k.end && k.end <= n && k.end - k.start <= max_len);
      CHECK(c == 0 || k.start >= ch[(size_t)c - 1].end);
      CHECK(k.first_segment >= 0 && k.n_segments >= 1 && k.first_segment + k.n_segments <= n_seg);
    }
    // probabilities shorter than the recording (a caller's detector that stopped early): the cut falls back, nothing is read behind them
    if (n_seg > 0 && n_probs > 8)
      CHECK(ohw_speech_chunks_host(seg.data(), n_seg, p.data(), n_probs / 8, fs, n, &plan, ch.data(), n_ch) >= 0);
    total_seg += (long)n_seg; total_ch += (long)n_ch;
  }
  // refusals
  float z[4] = {0.9f, 0.9f, 0.9f, 0.9f};
  ohw_speech_segment s1[1];
  ohw_speech_chunk c1[1];
  if (ohw_speech_segments_host(z, 4, 0, 640, nullptr, s1, 1) >= 0 || ohw_speech_segments_host(nullptr, 4, 160, 640, nullptr, s1, 1) >= 0 ||
      ohw_speech_segments_host(z, 4, 160, 640, nullptr, nullptr, 1) >= 0)
    return 2;
  s1[0].start = 10; s1[0].end = 5; s1[0].avg_probability = 0.f;
  if (ohw_speech_chunks_host(s1, 1, z, 4, 160, 640, nullptr, c1, 1) >= 0) return 3;
  ohw_vad_config any_length;
  ohw_default_vad_config(&any_length);
  any_length.min_speech_ms = 0;
  if (ohw_speech_segments_host(z, 4, 160, 640, &any_length, s1, 1) != 1 || s1[0].start != 0 || s1[0].end != 640) return 4;
  if (ohw_speech_chunks_host(s1, 1, z, 4, 160, 640, nullptr, c1, 1) != 1 || c1[0].start != 0 || c1[0].end != 640) return 5;
  std::printf("plan ok: %ld segments, %ld chunks\n", total_seg, total_ch);
  return 0;
}
