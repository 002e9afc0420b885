// host_engine.hpp — the engine object behind ohw_engine_* (host_engine.cpp: the C ABI, samplers, language tables, setters),
// its transcribe drivers (transcribe.cpp) and the multi-device pool (pool.cpp).
#pragma once
#include <string>
#include <thread>
#include <vector>

#include "common.hpp"

namespace ohw {
extern thread_local std::string g_last_error;
// a text lost `lead` bytes at its front and now holds new_len bytes: move and cut the spans that index it
void trim_spans(std::vector<ohw_span_time>& v, size_t lead, size_t new_len);
void trim_spans(std::vector<ohw_word_prob>& v, size_t lead, size_t new_len);

// one mark per window record: where the window's text starts in the UNTRIMMED text the spans index while a transcribe runs,
// and how many token times / words / segments it added (the pool re-indexes with these)
// n_token_probs / n_word_probs: the confidence entries it added (segment info: one per segment when confidence is on)
struct WindowMark { size_t text0 = 0; int32_t n_token_times = 0, n_words = 0, n_segments = 0, n_token_probs = 0, n_word_probs = 0; };

// what a transcribe accumulates window by window (TranscribeCall::emit appends to one): of the engine's last call, of one
// recording of a batch call, of the pool's gathered result
struct Transcript {
  std::string text;                               // untrimmed until trim()
  std::vector<int32_t> tokens;
  std::vector<ohw_window_quality> quality;        // one record per window
  std::vector<ohw_token_time> token_times;
  std::vector<ohw_span_time> words, segments;     // index text
  std::vector<ohw_token_prob> token_probs;        // confidence (ohw_engine_set_confidence): per kept text token of a scored window
  std::vector<ohw_word_prob> word_probs;          //   per word (indexes text)
  std::vector<ohw_segment_info> segment_info;     //   parallel to segments while confidence is on, else empty
  std::vector<WindowMark> marks;                  // one per window record
  std::vector<std::vector<int32_t>> contexts;     // per window record: what its T = 0 pass was decoded behind
  std::vector<ohw_command_hit> commands;          // per window record while a command list is set (ohw_engine_last_commands)
  void clear() { *this = Transcript(); }
  // reference :282-283: the text loses its leading and trailing white space; the spans then index the trimmed text
  void trim() {
    const size_t b0 = text.find_first_not_of(" \t\r\n"), b1 = text.find_last_not_of(" \t\r\n");
    text = b0 == std::string::npos ? std::string() : text.substr(b0, b1 - b0 + 1);
    trim_spans(words, b0 == std::string::npos ? 0 : b0, text.size());
    trim_spans(segments, b0 == std::string::npos ? 0 : b0, text.size());
    trim_spans(word_probs, b0 == std::string::npos ? 0 : b0, text.size());
  }
};
}  // namespace ohw

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
  // the seek loops
  int carry_max = 0;
  // ohw_engine_set_stitch: 0 off, else the overlap of neighbouring fixed cuts in ms; the seams and every window's kept tokens
  // (offsets: n_windows + 1 entries) of the last stitched transcribe
  int stitch_ms = 0;
  std::vector<ohw_seam> last_seams;
  std::vector<int32_t> last_win_tokens, last_win_offsets;
  int prefill_chunk = 8;                // ohw_engine_set_prefill_chunk: every state of the engine, those made later too
  int beam_size = 0;                     // ohw_engine_set_beam_size: 0 = greedy at T = 0, 2..5 = beam search (a decode batch then holds
                                         //   max_batch / beam_size windows, on the engine's own state)
  int best_of = 1;                       // ohw_engine_set_best_of: candidates per pending window on every rung above T = 0 (1: today's ladder)
  std::vector<int32_t> last_cands;       // ohw_engine_last_candidates: every best-of rung of the last transcribe
  std::vector<float> last_cand_lps;      //   and the candidates' log-probabilities, in the same order
  // ohw_engine_set_commands: the caller's index of every phrase of the list on the engine's state (the text form lists a text
  // in up to two forms)
  std::vector<int32_t> cmd_index;
  int force_len = 0;                     // measurement knob (ohw_engine_set_force_len): every window decodes exactly this many tokens
  // the last ohw_engine_transcribe: its records (words / segments index last_text once the call has trimmed) and the trimmed text
  ohw::Transcript last;
  std::string last_text;
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
  // ohw_engine_transcribe_batch / _long_batch: one record per recording, in submission order (ohw_engine_batch_result); its text
  // is trimmed.  lang_id: the language the recording was decoded in when it had one of its own (detected or caller-given), else -1
  // per_window (the long batch): ohw_engine_long_batch_quality / _context list the windows; the short batch has the one record
  struct BatchRecord {
    ohw::Transcript t; int32_t lang_id = -1; bool per_window = false;
    ohw_window_quality none{};          // what ohw_engine_batch_result points at for a recording that never ran a window
    size_t n_windows() const { return per_window ? t.quality.size() : 0; }
    // ohw_engine_transcribe_speech: the recording's speech segments and its chunks (one quality record per chunk)
    std::vector<ohw_speech_segment> speech;
    std::vector<ohw_speech_chunk> chunks;
  };
  std::vector<BatchRecord> batch_records;
  std::vector<std::vector<ohw_token_prob>> score_records;   // ohw_engine_score_batch: what its results point into, until the next call
  // ohw_engine_set_vad: what ohw_engine_transcribe_speech detects, segments and chunks with
  ohw_vad_config vad_cfg{0, 0.5f, 700, 250, 30};
  ohw_vad_detector vad_det{0.10f, 9.0f, 3.0f};
  ohw_chunk_plan chunk_plan{30.0f, 2000, 1100};
  // word timestamps (ohw_engine_set_word_timestamps): the heads every state of the engine aligns with (empty: off)
  std::vector<ohw_align_head> wt_heads;
  bool confidence = false;               // ohw_engine_set_confidence: every kept pass is scored by the unconstrained model (ohw_state_score)
  // language detection (ohw_engine_set_detect_language; only with language "auto" on a multilingual model).  given_lang: the pool
  // detected on its first engine and hands the id to this one (-1: detect yourself).  last_lang_id / last_lang_prob: what the
  // last transcribe decoded in and the detection's probability of it (1 when nothing was detected)
  bool detect_language = false;
  int32_t given_lang = -1;
  float given_prob = 0.f;
  int32_t last_lang_id = 0;
  float last_lang_prob = 1.f;
};


namespace ohw {
// an engine around an already loaded context (takes ownership of ctx on success); throws Error
ohw_engine* engine_wrap_ctx(ohw_ctx* ctx, const std::string& language, bool translate, int max_batch, int device);
// ---- the paths after validation (transcribe.cpp): windows, decode policy, text assembly; all throw Error ----
// one recording into e->last (untrimmed: the caller trims) and e->last_trace: the seek loop in OHW_WINDOW_SEEK, else fixed 30 s
// cuts.  win_first / win_step (fixed-cut modes only): the engine takes windows win_first, win_first + win_step, ... of the
// recording (the pool's round-robin deal); the records it leaves list its own windows in that order
void engine_transcribe(ohw_engine* e, const float* samples, int64_t n, int64_t win_first = 0, int64_t win_step = 1);
// n_recs validated recordings of at most one window each, batched longest first on the engine's own state and decoded by the
// same per-window code; fills e->batch_records.  langs (may be null): one language id or OHW_LANG_DETECT per recording
// t_offs (may be null: all 0): the offset of recording i on some longer recording's clock, in seconds, which its times are emitted
// with; trim = false leaves each record's text untrimmed (the speech call joins chunks first)
void engine_transcribe_batch(ohw_engine* e, const ohw_audio_span* recs, int n_recs, const int32_t* langs, const double* t_offs = nullptr,
                             bool trim = true);
// ohw_engine_score_batch after validation: engine_transcribe_batch's front end, then ohw_state_score on the caller's tokens
// (recording i: tokens[offsets[i] .. offsets[i + 1])); fills results and e->score_records
void engine_score_batch(ohw_engine* e, const ohw_audio_span* recs, int n_recs, const int32_t* tokens, const int32_t* offsets, ohw_score_result* results);
// speech-aware windows: detect (or take probs[i]), segment and chunk every validated recording, run all chunks as one
// engine_transcribe_batch, gather per recording; fills e->batch_records
void engine_transcribe_speech(ohw_engine* e, const ohw_audio_span* recs, const ohw_frame_probs* probs, int n_recs, const int32_t* langs);
// recordings of any length, each through the seek loop, one window of every live recording per round (ohw_seek_sched_*); the
// caller sets e->window_mode to OHW_WINDOW_SEEK for the call
void engine_transcribe_long_batch(ohw_engine* e, const ohw_audio_span* recs, int n_recs, const int32_t* langs);
// ---- pieces the entry points of the engine and of the pool share (host_engine.cpp) ----
// ohw_validate_audio or Error(OHW_E_VALIDATION, "Audio validation failed[ for recording <rec>]: <what>"); rec < 0: the only one
void validate_or_throw(const float* samples, int64_t n, uint32_t sample_rate, ohw_audio_info* info_out, int rec = -1);
// every entry of langs (may be null) is OHW_LANG_DETECT or an id of the model; `what` names the call in the message
void check_recording_langs(const char* what, const int32_t* langs, int n_recs, int n_langs);
// copy_text_out: text into a caller's buffer, truncated and NUL-terminated; write_language_out (out: null or >= 8 bytes): the configured code, or for "auto" the
// code of `id` (reference :288-296: whisper.cpp's default "en" -> 0, or what was detected)
void copy_text_out(char* buf, size_t cap, const std::string& text);
void write_language_out(char* out, const std::string& configured, int32_t id);
// the batch drivers run on the engine's own state with batch-invariant kernel selection; on the way out that goes off again and
// the language table (and, for the short batch, the per-window audio contexts) with it
struct BatchStateGuard {
  ohw_engine* e; bool window_ctx;
  BatchStateGuard(ohw_engine* e_, bool window_ctx_) : e(e_), window_ctx(window_ctx_) { (void)ohw_state_set_batch_invariant(e->state, 1); }
  ~BatchStateGuard() {
    if (window_ctx) (void)ohw_state_set_window_ctx(e->state, nullptr, 0);
    (void)ohw_state_set_batch_invariant(e->state, 0);
    (void)ohw_state_set_window_lang(e->state, nullptr, 0);
  }
};
// f(state) for the engine's own state, then for every state of the overlapped schedules (states[0] is the engine's own again)
template <typename F>
void each_state(const ohw_engine* e, F&& f) {
  f(e->state);
  for (ohw_state* st : e->states) f(st);
  for (ohw_state* st : e->lane_states) f(st);
}
// frees the states and streams of the overlapped schedules; the engine's own state stays
void engine_free_overlap(ohw_engine* e);
// does a transcribe of this engine detect?  (the setting, language "auto", a multilingual model)
bool engine_detects(const ohw_engine* e);
// the audio context of a call on n samples (ohw_engine_set_audio_ctx): the fixed one; auto = the context that covers a recording
// of at most one window, the full context (0) for anything longer
int engine_call_ctx(const ohw_engine* e, int64_t n);
// whisper.cpp detects once per whisper_full call, on the first window: the front end of window 0 of the recording alone on the
// engine's own state, under the context window 0 will be decoded in (recording-wide spectrogram in the recording-mel and seek
// modes), then ohw_state_detect_window_lang.  Returns the id, its probability in *prob; throws Error
int32_t engine_detect_first_window(ohw_engine* e, const float* samples, int64_t n, float* prob);
}  // namespace ohw
