// host_engine.hpp — the engine object behind ohw_engine_* (host_engine.cpp) and the multi-device pool (pool.cpp).
#pragma once
#include <string>
#include <thread>
#include <vector>

#include "common.hpp"

struct ohw_engine {
  ohw_ctx* ctx = nullptr;
  ohw_state* state = nullptr;
  std::string language;
  bool translate = false;
  int max_batch = 1;
  int window_mode = OHW_WINDOW_FIXED;
  int audio_ctx = 0;                     // ohw_engine_set_audio_ctx: 0 off (full context), n > 0 fixed, -1 auto
  bool packed_encoder = false;           // ohw_engine_set_packed_encoder: every state of the engine, those made later too
  // ohw_engine_set_initial_prompt: context tokens (clipped to the last n_text_ctx / 2 - 1) in front of every window of every
  // schedule; empty: none.  prompt_used: a prompt has been set at some time, so states may still hold a table to clear
  std::vector<int32_t> prompt;
  bool prompt_used = false;
  // ohw_engine_set_carry_context: 0 off, -1 the full cap, n > 0 at most n tokens of the recording's earlier windows as context in
  // the seek loops.  last_contexts: per window record of last_quality, what its T = 0 pass was decoded behind
  int carry_max = 0;
  int prefill_chunk = 8;                 // ohw_engine_set_prefill_chunk: every state of the engine, those made later too
  std::vector<std::vector<int32_t>> last_contexts;
  int beam_size = 0;                     // ohw_engine_set_beam_size: 0 = greedy at T = 0, 2..5 = beam search (a decode batch then holds
                                         //   max_batch / beam_size windows, on the engine's own state)
  int force_len = 0;                     // measurement knob (ohw_engine_set_force_len): every window decodes exactly this many tokens
  std::vector<int32_t> last_tokens;
  std::string last_text;
  std::vector<ohw_window_quality> last_quality;
  // two batches in flight for audio longer than max_batch windows (include/ohw.h, ohw_stream_create): a second state
  // and three streams, made on first use; enc_cus = 0 keeps the batches strictly one after the other
  std::vector<ohw_state*> states;        // states[0] == state; the others are made on the first long input
  std::vector<void*> lane_streams;       // LANES schedule: one CU-masked stream per decode lane
  std::vector<ohw_state*> lane_states;   //   and one state of max_batch * merge windows per lane
  int lane_capacity = 0;
  void* s_full = nullptr; void* s_enc = nullptr; void* s_dec = nullptr;
  int schedule = OHW_SCHEDULE_LANES;     // how audio longer than max_batch windows is overlapped (include/ohw.h)
  int lanes = 4;                         // decodes side by side in the LANES schedule
  int merge = 3;                         // batches of max_batch windows a lane takes through ONE front-end pass and ONE decode
  int enc_cus = 96;
  int device = 0;
  ohw_decode_policy policy{0.2f, 2.4f, -1.0f, 0.6f};
  bool fallback_device = false;          // the temperature ladder samples on the device (ohw_engine_set_fallback_device)
  std::vector<int32_t> last_trace;   // every decode pass of the last transcribe: {window, temperature * 1000, n, tokens...}
  // ohw_engine_transcribe_batch: one record per recording, in submission order (ohw_engine_batch_result)
  // lang_id: the language the recording was decoded in when it had one of its own (detected or caller-given), else -1
  struct BatchRecord {
    std::string text; std::vector<int32_t> tokens; ohw_window_quality quality{}; int32_t lang_id = -1;
    std::vector<ohw_window_quality> qualities;      // ohw_engine_transcribe_long_batch: one record per window (else empty)
    std::vector<std::vector<int32_t>> contexts;     //   and the context every window's T = 0 pass was decoded behind
    std::vector<ohw_token_time> token_times; std::vector<ohw_span_time> words, segments;
  };
  std::vector<BatchRecord> batch_records;
  // language detection (ohw_engine_set_detect_language; only with language "auto" on a multilingual model).  given_lang: the pool
  // detected on its first engine and hands the id to this one (-1: detect yourself).  last_lang_id / last_lang_prob: what the
  // last transcribe decoded in and the detection's probability of it (1 when nothing was detected)
  // word timestamps (ohw_engine_set_word_timestamps): the heads every state of the engine aligns with (empty: off), and the
  // times of the last transcribe; words / segments index last_text
  std::vector<ohw_align_head> wt_heads;
  std::vector<ohw_token_time> last_token_times;
  std::vector<ohw_span_time> last_words, last_segments;
  // one mark per window record of last_quality: where the window's text starts in the UNTRIMMED text the spans index while
  // engine_transcribe_core runs, and how many token times / words / segments it added (the pool re-indexes with these)
  struct WindowMark { size_t text0 = 0; int32_t n_token_times = 0, n_words = 0, n_segments = 0; };
  std::vector<WindowMark> last_marks;
  bool detect_language = false;
  int32_t given_lang = -1;
  float given_prob = 0.f;
  int32_t last_lang_id = 0;
  float last_lang_prob = 1.f;
};


namespace ohw {
// an engine around an already loaded context (takes ownership of ctx on success); throws Error
ohw_engine* engine_wrap_ctx(ohw_ctx* ctx, const std::string& language, bool translate, int max_batch, int device);
// the path after validation: windows, decode policy, text assembly (untrimmed text in *text); fills the engine's last_* records
// win_first / win_step (fixed-cut modes only): the engine takes windows win_first, win_first + win_step, ... of the recording
// (the pool's round-robin deal); the records it leaves (last_tokens / last_quality) list its own windows in that order
// recs != nullptr (ohw_engine_transcribe_batch; samples / n / text unused): n_recs validated recordings of at most one window each,
// batched longest first on the engine's own state and decoded by the same per-window code; fills e->batch_records
// rec_langs (with recs; may be null): one language id or OHW_LANG_DETECT per recording
// long_batch (with recs; ohw_engine_transcribe_long_batch): recordings of any length, each through the seek loop, one window of
// every live recording per round (ohw_seek_sched_*); the caller sets e->window_mode to OHW_WINDOW_SEEK for the call
void engine_transcribe_core(ohw_engine* e, const float* samples, int64_t n, std::string* text, int64_t win_first = 0, int64_t win_step = 1,
                            const ohw_audio_span* recs = nullptr, int n_recs = 0, const int32_t* rec_langs = nullptr, bool long_batch = false);
// a text lost `lead` bytes at its front and now holds new_len bytes: move and cut the spans that index it
void trim_spans(std::vector<ohw_span_time>& v, size_t lead, size_t new_len);
// does a transcribe of this engine detect?  (the setting, language "auto", a multilingual model)
bool engine_detects(const ohw_engine* e);
// whisper.cpp detects once per whisper_full call, on the first window: the front end of window 0 of the recording alone on the
// engine's own state, under the context window 0 will be decoded in (recording-wide spectrogram in the recording-mel and seek
// modes), then ohw_state_detect_window_lang.  Returns the id, its probability in *prob; throws Error
int32_t engine_detect_first_window(ohw_engine* e, const float* samples, int64_t n, float* prob);
}  // namespace ohw
