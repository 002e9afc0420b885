/*
 * ohw.h — C ABI of libohw.so, the MI355X-native Whisper hot path for OpenHush.
 *
 * This is the drop-in boundary.  The reference has no FFI of its own for this path: it calls
 * whisper.cpp through the `whisper-rs` crate (reference src/engine/whisper.rs:10-12).  Each entry
 * point below names the reference call site it replaces; INTEGRATION.md shows the Rust `extern "C"`
 * block and the `WhisperEngine` impl a maintainer would add on the reference side.
 *
 * Conventions
 *   - plain C, opaque handles, caller-allocated outputs, no exceptions/aborts across the boundary;
 *   - every function returns OHW_OK (0) or a negative code; ohw_last_error() gives the text of the
 *     last failure on the calling thread;
 *   - handles carry no thread affinity (the reference builds the engine on a tokio thread and
 *     moves it to the `transcription-worker` thread: reference src/queue/worker.rs:22,100-103);
 *     every call selects its device itself.  Calls on ONE state must be serial (the reference
 *     serialises with RefCell::borrow_mut, src/engine/whisper.rs:240);
 *   - the library fails loudly: no CPU fallback exists.  Without a usable gfx950 device
 *     ohw_ctx_create* returns OHW_E_NO_GPU (reference error taxonomy OH-3004).
 */
#ifndef OHW_H
#define OHW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OHW_ABI_VERSION 2

/* error codes: the negated OH-30xx taxonomy the reference documents
 * (reference .claude/knowledge/error-codes.md:79-104; WhisperError variants src/engine/whisper.rs:14-27) */
enum {
  OHW_OK = 0,
  OHW_E_MODEL_NOT_FOUND = -3001, /* WhisperError::ModelNotFound   */
  OHW_E_LOAD_FAILED = -3002,     /* WhisperError::LoadFailed      */
  OHW_E_TRANSCRIBE = -3003,      /* WhisperError::TranscriptionFailed */
  OHW_E_NO_GPU = -3004,
  OHW_E_OOM = -3005,
  OHW_E_INVALID_ARG = -3006,
  OHW_E_VALIDATION = -3007       /* WhisperError::ValidationFailed (code in ohw_audio_info.error) */
};

/* compute dtype of weights/activations fed to MFMA (accumulation, LN, softmax, logits: fp32) */
/* OHW_DTYPE_AUTO (ohw_ctx_create / ohw_engine_new / ohw_pool_create only): f16 when the file stores f16 weights (ftype 1, the
 * stock ggml-*.bin files: the weights stay exact), bf16 for f32 files.  BASELINE.json's bench dtype is bf16, chosen explicitly.
 * A quantised file (ftype 2, 3, 7, 8, 9) picks f16 as well: ggml expands its blocks to f16 / f32, and bf16 would drop three
 * more mantissa bits of every expanded weight for nothing. */
enum { OHW_DTYPE_AUTO = -1, OHW_DTYPE_BF16 = 0, OHW_DTYPE_F16 = 1 };

/* log-mel tail convention */
enum { OHW_MEL_REFLECT = 0 /* feature-extractor convention, pinned by goldens */,
       OHW_MEL_ZERO_TAIL = 1 /* whisper.cpp convention: zeros after the audio */ };

typedef struct ohw_ctx ohw_ctx;     /* model: weights resident in HBM  (whisper-rs WhisperContext) */
typedef struct ohw_state ohw_state; /* activations, KV caches, streams  (whisper-rs WhisperState)   */

typedef struct {
  int32_t n_vocab, n_audio_ctx, n_audio_state, n_audio_head, n_audio_layer;
  int32_t n_text_ctx, n_text_state, n_text_head, n_text_layer, n_mels, ftype;
} ohw_hparams;

typedef struct {
  int32_t eot, sot, translate, transcribe, solm, prev, nosp, no_timestamps, timestamp_begin, blank;
  int32_t n_langs;
} ohw_special_tokens;

/* ---- audio validation: reference src/engine/validation.rs:46-118 (validate_audio) ------------- */
enum { OHW_AUDIO_OK = 0, OHW_AUDIO_EMPTY = 1, OHW_AUDIO_BAD_RATE = 2, OHW_AUDIO_TOO_LONG = 3,
       OHW_AUDIO_TOO_SHORT = 4, OHW_AUDIO_NAN = 5, OHW_AUDIO_INF = 6 };
typedef struct {
  int32_t error;          /* OHW_AUDIO_* */
  float duration_secs;
  int64_t sample_count;
  float min_value, max_value, rms;
  int64_t nan_count, inf_count;
} ohw_audio_info;
/* host-side scan, same order of checks and same arithmetic as the reference */
int ohw_validate_audio(const float* samples, int64_t n, uint32_t sample_rate, ohw_audio_info* info);

/* ---- model: replaces WhisperContext::new_with_params (reference src/engine/whisper.rs:156-160) - */
/* model_path: a ggml `ggml-*.bin` file (reference src/engine/whisper.rs:71-79).  A missing file   */
/* returns OHW_E_MODEL_NOT_FOUND before any device work (reference :141-154, test :984-997).       */
/* Tensors may be f32, f16 or block-quantised Q4_0 / Q4_1 / Q5_0 / Q5_1 / Q8_0 (ttype 0, 1, 2, 3, 6, 7, 8; a file may mix):  */
/* quantised blocks are uploaded as stored and expanded on the device at load, so the resident weights, their footprint   */
/* and the throughput are those of an f16 file.  The header's ftype word is ftype + 1000 * quantisation version;          */
/* ohw_hparams.ftype holds the reduced ftype.  k-quants and quantisation versions other than 2: OHW_E_LOAD_FAILED.        */
/* Accepted dimensions (every ohw_ctx_create* entry; anything else: OHW_E_LOAD_FAILED "unsupported model dimensions: ..."): */
/* n_text_state == n_audio_state, a multiple of 128 from 128 to 1280 (the decoder's fused LayerNorm holds 1280 columns),   */
/* d_head 64 (n_*_head * 64 == n_*_state), n_audio_ctx 1500, n_text_ctx <= 448, n_mels <= 128, 1 .. 64 layers each side.   */
int ohw_ctx_create(const char* model_path, int device, int dtype, ohw_ctx** out);
/* procedural weights generated on the device (tests / bench; openhush_amd/synth.py is the spec)  */
int ohw_ctx_create_synthetic(const ohw_hparams* hp, uint32_t seed, int device, int dtype, ohw_ctx** out);
int ohw_ctx_info(const ohw_ctx* ctx, ohw_hparams* hp, ohw_special_tokens* tok);
int ohw_ctx_dtype(const ohw_ctx* ctx);   /* the 16-bit type the context computes in (what OHW_DTYPE_AUTO resolved to) */
/* ---- a loaded model as ONE device blob: the rank that read the file exports it, the caller broadcasts it (RCCL) and
 *      the other ranks import it into a shell context made from the same hparams and dtype - instead of every rank
 *      reading and repacking the file ("one ncclBroadcast of the packed weight blob at load").  A shell has
 *      no vocabulary strings: the exporting rank detokenises. ------------------------------------------------------ */
int ohw_ctx_create_shell(const ohw_hparams* hp, int device, int dtype, ohw_ctx** out);
size_t ohw_ctx_blob_size(const ohw_ctx* ctx);
int ohw_ctx_blob_export(const ohw_ctx* ctx, void* dst_device, size_t capacity);
int ohw_ctx_blob_import(ohw_ctx* ctx, const void* src_device, size_t bytes);
/* bytes of token `id` (text tokens only); returns length, 0 for specials                         */
int ohw_token_text(const ohw_ctx* ctx, int32_t id, const char** text);
void ohw_ctx_free(ohw_ctx* ctx); /* WhisperContext drop */

/* ---- audio preprocessing, the step right before the path (host code: the envelope follower and the
 *      limiter are sequential recurrences over the whole recording).  In place, fp32, the reference's operation order:
 *      AudioBuffer::{rms_db, apply_gain, normalize_rms, compress, limit} (reference src/input/audio.rs:86-239),
 *      resample_linear (:972-990), TranscriptionWorker::preprocess_audio (src/queue/worker.rs:196-240).  The rubato sinc
 *      resampler is restated below (ohw_dsp_resample_sinc, ohw_resampler_*).  RNNoise: everything AudioBuffer::denoise
 *      does around the network is built (ohw_dsp_denoise); the network itself (nnnoiseless 0.5.2, a third-party crate with
 *      trained weights that is not in the reference tree) plugs in through ohw_denoise_engine. ------------------------- */
typedef struct ohw_preprocess_config {
  int32_t preprocessing;              /* master switch, reference default 0 (src/config.rs:958,984) */
  int32_t normalization_enabled; float normalization_target_db;                       /* 1, -18 dB */
  int32_t compression_enabled; float compression_threshold_db, compression_ratio,     /* 1, -24 dB, 4:1, */
      compression_attack_ms, compression_release_ms, compression_makeup_gain_db;      /* 5 ms, 50 ms, +6 dB */
  int32_t limiter_enabled; float limiter_ceiling_db, limiter_release_ms;              /* 1, -1 dB, 50 ms */
} ohw_preprocess_config;
void ohw_default_preprocess_config(ohw_preprocess_config* c);
int ohw_preprocess_audio(float* samples, int64_t n, uint32_t sample_rate, const ohw_preprocess_config* c);
/* The noise-reduction stage of the chain (BASELINE config #5 names it; reference src/input/audio.rs:249-341, called first and
 * independently of the `preprocessing` switch: src/queue/worker.rs:197-207).  ohw_denoise_engine is what a host plugs its
 * nnnoiseless::DenoiseState into: process_frame takes ONE 480-sample frame at 48 kHz scaled to the 16-bit range (x 32767,
 * as DenoiseState::process_frame does), writes 480 samples and returns the frame's voice probability; reset (may be NULL)
 * stands for DenoiseState::new() and is called once per ohw_dsp_denoise.  ohw_dsp_denoise does the rest in the reference's
 * order: linear resampling to 48 kHz (resample_for_rnnoise :996-1001), zero-padded last frame, first frame faded in, only
 * the real part of a short last frame kept, linear resampling back, truncate / zero-extend to n, mix by `strength` in 0..1. */
typedef struct ohw_denoise_engine {
  void* user;
  float (*process_frame)(void* user, float* out480, const float* in480);
  void (*reset)(void* user);
} ohw_denoise_engine;
int ohw_dsp_denoise(float* samples, int64_t n, uint32_t sample_rate, float strength, const ohw_denoise_engine* engine);
void ohw_denoise_passthrough_engine(ohw_denoise_engine* e);   /* out = in: the chain's framing without a network (tests) */
/* preprocess_audio with the reference's noise_reduction settings (src/config.rs NoiseReductionConfig {enabled, strength}):
 * enabled != 0 needs an engine (OHW_E_INVALID_ARG without one - never a silent skip) */
int ohw_preprocess_audio_ex(float* samples, int64_t n, uint32_t sample_rate, const ohw_preprocess_config* c,
                            int noise_reduction_enabled, float noise_reduction_strength, const ohw_denoise_engine* denoise);
float ohw_dsp_rms_db(const float* samples, int64_t n);                 /* -inf for silence / empty */
void ohw_dsp_apply_gain(float* samples, int64_t n, float gain_db);
void ohw_dsp_normalize_rms(float* samples, int64_t n, float target_db);
void ohw_dsp_compress(float* samples, int64_t n, uint32_t sample_rate, float threshold_db, float ratio, float attack_ms,
                      float release_ms, float makeup_gain_db);
int64_t ohw_dsp_limit(float* samples, int64_t n, uint32_t sample_rate, float ceiling_db, float release_ms); /* samples over the ceiling */
/* returns the output length; with out == NULL or out_cap too small nothing is written (size query) */
int64_t ohw_dsp_resample_linear(const float* in, int64_t n, uint32_t from_rate, uint32_t to_rate, float* out, int64_t out_cap);

/* high-quality resampling: the reference's resample(.., ResamplingQuality::High) = rubato's SincFixedIn with sinc_len 256,
 * f_cutoff 0.95, oversampling 256, linear interpolation between sub-filters, BlackmanHarris2 window, fed in chunks of 1024
 * input samples (reference src/input/audio.rs:1007-1095).  The rubato crate is not in the reference tree: the algorithm is
 * restated from its published design (windowed-sinc polyphase table, two nearest sub-filters blended linearly), parity
 * unpinned.  Same size-query convention as ohw_dsp_resample_linear.                                                  */
int64_t ohw_dsp_resample_sinc(const float* in, int64_t n, uint32_t from_rate, uint32_t to_rate, float* out, int64_t out_cap);

/* the same resampler on the device (resample.hip): every output sample is independent, so a recording that lies in HBM - or
 * goes there for the log-mel anyway - is resampled there (one wave per output sample; 30 s at 48 kHz in a fraction of a
 * millisecond).  Same number of samples as ohw_dsp_resample_sinc and, up to the order of the fp32 sums, the same samples.
 *   ohw_resampler_create     builds the 256 x 256 polyphase table for from_rate -> to_rate on `device`;
 *   ohw_resampler_out_len    output samples for n input samples;
 *   ohw_resampler_run        in / out in host or device memory (in_on_device / out_on_device), on hip_stream (NULL = the
 *                            default stream); returns when host buffers may be reused, asynchronous when both are device.
 * One call at a time per handle (it stages host buffers in the handle's own device memory); handles are independent. */
typedef struct ohw_resampler ohw_resampler;
int ohw_resampler_create(int device, uint32_t from_rate, uint32_t to_rate, ohw_resampler** out);
void ohw_resampler_free(ohw_resampler* r);
int64_t ohw_resampler_out_len(const ohw_resampler* r, int64_t n);
int ohw_resampler_run(ohw_resampler* r, const float* in, int64_t n, int in_on_device, float* out, int64_t out_cap, int out_on_device,
                      void* hip_stream);

/* ---- voice-activity segmentation, the step in front of the path in continuous mode (host code) --------
 *      ohw_vad_state_*: the reference's VadState (src/vad/mod.rs:112-250) - per-chunk VAD results in, speech segments out;
 *      ohw_vad_engine: its VadEngine trait (src/vad/mod.rs:34-55) as a struct of function pointers, so the host plugs in the
 *      detector (the reference's SileroVad needs an ONNX model that is not available offline); ohw_vad_run: the daemon's
 *      continuous-mode loop over a recording (src/daemon.rs:2062-2138); ohw_vad_energy_engine: a built-in short-time-energy
 *      detector for tests and model-less hosts (not Silero). ------------------------------------------------------------ */
typedef struct { int32_t enabled; float threshold; uint32_t min_silence_ms, min_speech_ms, speech_pad_ms; } ohw_vad_config;
void ohw_default_vad_config(ohw_vad_config* c);     /* 0, 0.5, 700, 250, 30 (reference src/vad/mod.rs:76-100) */
typedef struct { int64_t start, end; float avg_probability; } ohw_speech_segment;   /* positions in samples */
typedef struct ohw_vad_state ohw_vad_state;
ohw_vad_state* ohw_vad_state_new(const ohw_vad_config* cfg, uint32_t sample_rate);
void ohw_vad_state_free(ohw_vad_state* s);
/* returns 1 and fills *seg when a speech segment just ended, 0 otherwise, negative on a bad argument */
int ohw_vad_state_update(ohw_vad_state* s, float probability, int is_speech, int64_t chunk_samples, ohw_speech_segment* seg);
int ohw_vad_state_is_speech(const ohw_vad_state* s);
int64_t ohw_vad_state_speech_start(const ohw_vad_state* s);   /* -1 when not in speech */
void ohw_vad_state_reset(ohw_vad_state* s);
typedef struct {
  void* user;
  int (*process)(void* user, const float* samples, int64_t n, float* probability);   /* 0 = ok; 16 kHz mono f32 */
  void (*reset)(void* user);                                                           /* may be NULL */
  int32_t chunk_size;     /* 512 for Silero */
  uint32_t sample_rate;   /* 16000 */
} ohw_vad_engine;
int ohw_vad_energy_engine(float threshold_db, ohw_vad_engine* out);
void ohw_vad_energy_engine_free(ohw_vad_engine* e);
/* number of speech segments of a recording (all of them; at most cap are written to out), or a negative error code */
int64_t ohw_vad_run(const ohw_vad_engine* engine, const ohw_vad_config* cfg, const float* samples, int64_t n, int64_t poll_samples,
                    ohw_speech_segment* out, int64_t cap);

/* ---- speech-aware windows: a device detector, a host plan, and (further down) ohw_engine_transcribe_speech -------------
 * The three rules below are THIS PROJECT'S OWN definitions.  None of them is the reference's (its VadState and daemon loop are
 * the entries above) and the detector is not Silero: it is a model-free spectral rule and makes no claim to Silero's accuracy on
 * real speech, which is unmeasured.  A host that has Silero hands its own probabilities to the plan instead (frame_samples 512).
 *
 * DETECTOR  ohw_state_vad_frames: one speech probability per 10 ms frame of a recording that ohw_validate_audio accepts, 16 kHz
 * mono.  pcm: host or device samples (pcm_on_device, as ohw_mel); prob_out: HOST array of n_frames = (n + 159) / 160 floats;
 * floor_db_out (or NULL): the noise floor.  The call uses scratch buffers of its own and leaves the state's recording, slots,
 * mel and graphs alone.  Three launches on the state's stream (vad.hip):
 *   band   frame t = 400 samples centred at t * 160 under the periodic Hann window of the mel front end; samples are reflected at
 *          the recording's start only and are zero from n on;  e[t] = 10 * log10(max(sum_{k = 8..85} |X_t[k]|^2, 1e-10)), fp32:
 *          the 320 .. 3400 Hz band of the 400-point DFT
 *   floor  a histogram of e in 320 bins of 0.5 dB from -100 dB, bin = clamp((int)floorf((e + 100) * 2), 0, 319); the noise floor is
 *          the lower edge of the first bin whose cumulative count reaches ceilf(floor_quantile * n_frames) (fp32; at least 1)
 *   prob   es[t] = the mean of e over the frames of [t - 2, t + 2] that exist, summed in ascending order;
 *          p[t] = 1 / (1 + exp(-(es[t] - floor - margin_db) / slope_db))
 * ohw_default_vad_detector: 0.10, 9, 3.  floor_quantile in (0, 1], slope_db > 0, all three finite, else OHW_E_INVALID_ARG.     */
typedef struct { float floor_quantile, margin_db, slope_db; } ohw_vad_detector;
void ohw_default_vad_detector(ohw_vad_detector* d);
int ohw_state_vad_frames(ohw_state* st, const float* pcm, int64_t n, int pcm_on_device, const ohw_vad_detector* d, float* prob_out,
                         float* floor_db_out);
/* SEGMENTS  ohw_speech_segments_host (host only, no device): per-frame probabilities -> speech segments, modelled on Silero's
 * get_speech_timestamps with ohw_vad_config's fields, `enabled` ignored.  Frame f covers samples [f * frame_samples,
 * (f + 1) * frame_samples); frame_samples is 160 for the detector above, 512 for Silero.  neg = max(threshold - 0.15, 0.01);
 * min_silence / min_speech / pad in samples = ms * 16.  Frames in order: p >= threshold opens a segment if none is open and
 * clears a pending end; in an open segment p < neg sets a pending end at that frame if none is set; once the frames from the
 * pending end through the current one cover min_silence ((f + 1 - pending) * frame_samples >= min_silence) the segment closes
 * at the pending end and is kept if (end - start) * frame_samples >= min_speech; at the end an open segment closes at n_probs under the same
 * test.  Then every kept segment grows by the pad on both sides, neighbours whose pads would meet (gap < 2 * pad) share the gap
 * at its midpoint (gap / 2 to the earlier one), and everything is clipped to [0, n_samples].  avg_probability: the mean of p
 * over the unpadded frames.  Returns the number of segments (all of them; at most cap are written), or a negative error code.  */
int64_t ohw_speech_segments_host(const float* probs, int64_t n_probs, int frame_samples, int64_t n_samples, const ohw_vad_config* cfg,
                                 ohw_speech_segment* out, int64_t cap);
/* CHUNKS  ohw_speech_chunks_host (host only): segments -> contiguous spans of the recording of at most max_chunk_s, each one
 * recording of a batch.  Segments in order; a new chunk starts when the gap to the previous segment exceeds max_gap_ms or when
 * the span from the chunk's start to this segment's end would exceed max_chunk_s.  A single segment longer than max_chunk_s is
 * cut at the frame of lowest p in [start + max_chunk_s / 2, start + max_chunk_s) (frames that start in that range; the first
 * minimum; no pad at the cut; the cut is at that frame's first sample) and the rule repeats on the rest; a piece in front of
 * a cut is a chunk of its own, the rest starts a new chunk that later segments may join; with no frame in that range the cut is
 * at start + max_chunk_s.  A chunk shorter than min_chunk_ms grows evenly on both sides into the surrounding audio,
 * bounded by its neighbours and by the recording.  first_segment / n_segments: the segments a chunk holds (a cut segment counts
 * in each of its pieces).  ohw_default_chunk_plan: 30, 2000, 1100.  min_chunk_ms stays above 1000: the batch path drops a cut of
 * at most 100 frames of 10 ms (like a call with less than 1 s of audio), which would lose a short chunk's text.
 * max_chunk_s in (0, 30].  Returns the number of chunks (at most cap are written), or a negative error code.                    */
typedef struct { float max_chunk_s; uint32_t max_gap_ms, min_chunk_ms; } ohw_chunk_plan;
typedef struct { int64_t start, end; int32_t first_segment, n_segments; } ohw_speech_chunk;   /* positions in samples */
void ohw_default_chunk_plan(ohw_chunk_plan* p);
int64_t ohw_speech_chunks_host(const ohw_speech_segment* segments, int64_t n_seg, const float* probs, int64_t n_probs, int frame_samples,
                               int64_t n_samples, const ohw_chunk_plan* plan, ohw_speech_chunk* out, int64_t cap);

/* ---- streaming glue right after the path, host code -----------------------------------------------
 *      ohw_tracker_*: TranscriptionTracker (reference src/queue/mod.rs:59-297) - chunks are registered as pending under
 *      back-pressure, results come back in any order, take_ready releases them (streaming mode: all completed chunks sorted
 *      by (sequence, chunk), the words that repeat the end of the previous output removed; ordered mode: recordings in
 *      sequence order).  ohw_extract_chunk: AudioRecorder::extract_chunk for a 16 kHz recorder (src/input/audio.rs:737-785:
 *      nothing below 0.1 s, zero padding to 1.1 s).  ohw_chunk_scheduler_*: the chunk-timer arm of the daemon loop
 *      (src/daemon.rs:1958-2011).  Strings are UTF-8; a text returned by ohw_tracker_ready_get lives until the next
 *      take_ready on that tracker.  A tracker or scheduler is used by one thread at a time (the reference holds its tracker
 *      inside the daemon's loop); they touch no device. */
enum { OHW_BACKPRESSURE_WARN = 0, OHW_BACKPRESSURE_DROP_OLDEST = 1, OHW_BACKPRESSURE_DROP_NEWEST = 2 };
typedef struct ohw_tracker ohw_tracker;
ohw_tracker* ohw_tracker_new(int streaming);
void ohw_tracker_free(ohw_tracker* t);
/* 1 = accepted, 0 = refused (DROP_NEWEST at max_pending), negative = error; max_pending 0 = unlimited */
int ohw_tracker_add_pending(ohw_tracker* t, uint64_t sequence_id, uint32_t chunk_id, uint32_t max_pending, uint32_t high_water_mark, int strategy);
int ohw_tracker_add_result(ohw_tracker* t, const char* text, uint64_t sequence_id, uint32_t chunk_id, int is_final, float duration_secs);
int ohw_tracker_take_ready(ohw_tracker* t);   /* number of released results, read with ohw_tracker_ready_get(t, 0 .. n-1, ..) */
int ohw_tracker_ready_get(const ohw_tracker* t, int i, const char** text, uint64_t* sequence_id, uint32_t* chunk_id, int* is_final,
                          float* duration_secs);
void ohw_tracker_reset_dedup(ohw_tracker* t);
int ohw_tracker_is_empty(const ohw_tracker* t);
int ohw_tracker_is_pending(const ohw_tracker* t, uint64_t sequence_id, uint32_t chunk_id);
int ohw_tracker_pending_count(const ohw_tracker* t);
int ohw_tracker_waiting_count(const ohw_tracker* t);
/* length of the chunk [from_pos, to_pos) after padding (0: shorter than 0.1 s); written to out when out_cap suffices */
int64_t ohw_extract_chunk(const float* recording, int64_t n_recording, int64_t from_pos, int64_t to_pos, float* out, int64_t out_cap);
typedef struct ohw_chunk_scheduler ohw_chunk_scheduler;
ohw_chunk_scheduler* ohw_chunk_scheduler_new(ohw_tracker* tracker, uint64_t sequence_id, uint32_t max_pending, uint32_t high_water_mark,
                                             int strategy);
void ohw_chunk_scheduler_free(ohw_chunk_scheduler* s);
/* one timer tick at recorder position current_pos: the job's length (its samples: ohw_extract_chunk(*from_pos, current_pos)) and
 * id, or 0 - too short (nothing moved) or refused by the tracker (position and id moved on, as in the reference) */
int64_t ohw_chunk_scheduler_tick(ohw_chunk_scheduler* s, const float* recording, int64_t n_recording, int64_t current_pos,
                                 uint32_t* chunk_id, int64_t* from_pos);
int64_t ohw_chunk_scheduler_position(const ohw_chunk_scheduler* s);
uint32_t ohw_chunk_scheduler_next_id(const ohw_chunk_scheduler* s);
int64_t ohw_chunk_scheduler_rejected(const ohw_chunk_scheduler* s);

/* ---- state: replaces ctx.create_state() (reference src/engine/whisper.rs:167-169) ------------- */
/* max_batch = number of independent 30 s windows processed together (the reference: 1)           */
int ohw_state_create(ohw_ctx* ctx, int max_batch, ohw_state** out);
void ohw_state_free(ohw_state* st); /* WhisperState drop: frees all device memory */
/* HIP stream (hipStream_t) every later call on this state enqueues on; NULL = the state's own    */
int ohw_state_set_stream(ohw_state* st, void* hip_stream);
int ohw_state_max_batch(const ohw_state* st);
const ohw_ctx* ohw_state_ctx(const ohw_state* st);

/* ---- streams for two batches in flight (the reference has one state and no overlap: src/queue/worker.rs:100-160
 *      transcribes one buffer at a time).  The encoder is MFMA-bound and the decoder HBM/latency-bound, so the engine
 *      runs the encoder of batch i+1 beside the decoder of batch i on DISJOINT sets of compute units: a stream made here
 *      is restricted to CU-mask bits [first_cu, first_cu + n_cu) (bits are dealt round-robin over the 8 XCDs, so any
 *      contiguous range is spread evenly; a mask that would leave an XCD without any CU is not honoured by the
 *      runtime - tools/probes/xcd_mask_probe.hip - so whole-XCD partitions cannot be made); n_cu = 0 makes an unrestricted stream.  ohw_stream_wait makes `waiter` wait
 *      for everything enqueued on `signal` so far (event record + wait, no host sync). ------------------------------- */
int ohw_stream_create(int device, int first_cu, int n_cu, void** stream_out);
int ohw_stream_destroy(void* stream);
int ohw_stream_wait(void* waiter, void* signal);
int ohw_stream_sync(void* stream);

/* ---- the stages of state.full() (reference src/engine/whisper.rs:266-268), split so that the   */
/*      host keeps windowing and sampling (BASELINE.json north_star) ------------------------------ */

/* log-mel of `batch` windows.  pcm: batch rows of `pcm_stride` floats (host memory, or device     */
/* memory when pcm_on_device != 0); n_samples[b] <= 480000 valid samples per row (rest = silence). */
/* mel_out (optional, host or NULL): [batch][n_mels][3000] f32 copy of the normalised log-mel.     */
int ohw_mel(ohw_state* st, const float* pcm, int64_t pcm_stride, const int32_t* n_samples, int batch,
            int pcm_on_device, int mel_mode, float* mel_out);

/* The spectrogram of a WHOLE recording, windows cut from it afterwards - what whisper.cpp does inside state.full() for
 * audio of any length (whisper_pcm_to_mel on all samples, then the encoder reads 3000 frames at the seek offset; reference
 * src/engine/whisper.rs:266-268 hands the whole buffer over).  Against ohw_mel on the samples from the seek offset on, a
 * window gets (a) the clamp `max - 8` from the maximum over ALL frames of the recording, (b) real neighbouring samples at
 * its edges (the 200-sample reflection only at the recording's start, zeros only after its end).
 *   ohw_recording_set: copies the recording (host, or device when pcm_on_device != 0; 1 .. 2 h of 16 kHz samples) into
 *     the state and finds that maximum in one pass (log_max_out, optional: log10 of the largest mel power);
 *   ohw_mel_seek: windows [seek_frames[b], +3000) (10 ms frames) of that spectrogram, for ohw_encode(batch) as after
 *     ohw_mel; mel_out as there.  The engine's OHW_WINDOW_SEEK mode runs on these two. */
int ohw_recording_set(ohw_state* st, const float* pcm, int64_t n, int pcm_on_device, float* log_max_out);
int ohw_mel_seek(ohw_state* st, const int32_t* seek_frames, int batch, float* mel_out);
/* Recording slots: a state holds up to max_batch recordings side by side, next to the single one above (which keeps its
 * behaviour and its bits), so that one window of each of several recordings can go through one encode and one decode batch.
 *   ohw_recording_set_slot: ohw_recording_set into slot `slot` (0 .. max_batch - 1), with the same limits per slot; the
 *     recording's own log-mel maximum is found in one pass and kept in that slot's entry of a per-slot table.  Setting a slot
 *     again replaces its recording (a shorter one never sees the old samples: every read is bounded by the new length).
 *   ohw_mel_seek_slots: window b is frames [seek_frames[b], +3000) of the spectrogram of the recording in slots[b], clamped
 *     with THAT recording's maximum, reflected only at that recording's start, zeros only after that recording's end.  A slot
 *     may appear more than once.  An empty slot, a slot outside the state, or a seek outside that recording's frames returns
 *     OHW_E_INVALID_ARG.  Afterwards the state is as after ohw_mel_seek(batch): ready for ohw_encode(batch), under the same
 *     ohw_state_set_audio_ctx / ohw_state_set_window_ctx rules.
 * The arithmetic is ohw_recording_set's / ohw_mel_seek's: a window is bit-identical to the one those two give for the same
 * recording and seek.  Slot storage is allocated when a slot is first set, sized by the largest recording the state has seen;
 * a state that never sets a slot allocates nothing. */
int ohw_recording_set_slot(ohw_state* st, int slot, const float* pcm, int64_t n, int pcm_on_device, float* log_max_out);
int ohw_mel_seek_slots(ohw_state* st, const int32_t* slots, const int32_t* seek_frames, int batch, float* mel_out);
/* encoder + cross-attention K/V of every decoder layer, for the windows of the last ohw_mel      */
int ohw_encode(ohw_state* st, int batch);
/* the same into windows [first, first + batch) of a decode batch of `total` windows (total <= max_batch): several front-end
 * passes can feed ONE decode - the decoder streams its weights once per step whatever its batch, so four 32-window front ends
 * decoded as one 128-row batch move 13 % fewer bytes per token than four 32-row decodes.  ohw_greedy / ohw_decode /
 * ohw_beam_search then take batch = total.                                                                          */
int ohw_encode_slice(ohw_state* st, int batch, int first, int total);
/* feed tokens[b][0..n_new) at positions n_past[b].. and return logits of the last fed position    */
/* per window: logits_out [batch][n_vocab] f32 (host).  tokens: [batch][n_new] row-major.          */
int ohw_decode(ohw_state* st, const int32_t* tokens, int n_new, const int32_t* n_past, int batch, float* logits_out);
/* the same for a SUBSET of the batch: windows with active[b] == 0 ride along (their rows of the weight-streaming GEMMs cost
 * nothing) but their cross K/V is not streamed and their logits row is not copied.  What the temperature fallback uses to
 * re-decode only the windows that failed, on their resident cross K/V.  active == NULL: every window.              */
int ohw_decode_active(ohw_state* st, const int32_t* tokens, int n_new, const int32_t* n_past, int batch, const int32_t* active,
                      float* logits_out);

/* language identification for the windows of the last ohw_encode (whisper.cpp whisper_lang_auto_detect: one
 * decoder step on [sot], soft-max over the language tokens only).  lang_ids_out [batch];
 * lang_probs_out [batch][n_langs] or NULL.  The reference never enables auto-detection ("auto" keeps
 * whisper.cpp's default "en": SURVEY.md section 0 item 6); this entry point exists for SURVEY.md row A4.8. */
int ohw_detect_language(ohw_state* st, int batch, int32_t* lang_ids_out, float* lang_probs_out);

/* sampling parameters: the whisper.cpp defaults the reference inherits because it sets none     */
/* (reference src/engine/whisper.rs:243-263)                                 */
typedef struct {
  int32_t lang_id;        /* 0 = "en": what language "auto" means in the reference */
  int32_t translate;      /* task token; the reference passes !config.translate (whisper.rs:251-257) */
  int32_t no_timestamps;  /* 0 */
  int32_t suppress_blank; /* 1 */
  int32_t max_initial_ts; /* 50 = 1.0 s / 0.02 s */
  int32_t n_max;          /* n_text_ctx/2 - 4 = 220 */
  int32_t force_len;      /* > 0: EOT suppressed, decoding stops after exactly this many tokens    */
} ohw_sample_params;
void ohw_default_sample_params(const ohw_ctx* ctx, ohw_sample_params* p);

/* host-side logits filter + arg-max for one window (the "token sampler" the host owns).          */
/* logits: [n_vocab], modified in place; cur: tokens sampled so far in this window.               */
int32_t ohw_sample_greedy_host(const ohw_ctx* ctx, const ohw_sample_params* p, float* logits,
                               const int32_t* cur, int n_cur, float* logprob_out);

/* the host sampler at a temperature: whisper.cpp's whisper_sample_token(best = false) - logits / temperature, the same
 * filter, then one draw of std::discrete_distribution over exp(logprobs) from a std::mt19937 (whisper.cpp seeds each
 * decoder's generator with 0 once per whisper_full call).  temperature <= 0: arg-max (rng may be NULL).
 * no_speech_prob_out (may be NULL) is written on a window's first step (n_cur == 0): soft-max probability of the
 * no-speech token in the scaled, unfiltered row.                                                                    */
typedef struct ohw_rng ohw_rng;
ohw_rng* ohw_rng_new(uint32_t seed);
void ohw_rng_free(ohw_rng* rng);
int32_t ohw_sample_host(const ohw_ctx* ctx, const ohw_sample_params* p, float* logits, const int32_t* cur, int n_cur,
                        float temperature, ohw_rng* rng, float* logprob_out, float* no_speech_prob_out);
/* the draws of a generator, for a sampler that is not on the host: one draw of std::discrete_distribution is one
 * std::generate_canonical<double, 53> (two engine outputs), compared against the normalised partial sums.
 * ohw_rng_uniforms writes the next n canonical doubles, drawn from a COPY of the generator (rng does not advance);
 * ohw_rng_discard_draws advances rng by n draws, where n calls of ohw_sample_host at T > 0 would leave it.             */
int ohw_rng_uniforms(const ohw_rng* rng, int n, double* out);
int ohw_rng_discard_draws(ohw_rng* rng, int n);

/* device-resident greedy loop for the windows of the last ohw_encode: prompt, KV-cached steps,   */
/* logits filter and arg-max all stay on the GPU; only token ids come back.                        */
/* tokens_out [batch][max_tokens] i32, n_tokens_out [batch] (host); EOT is not stored.             */
int ohw_greedy(ohw_state* st, const ohw_sample_params* p, int batch, int32_t* tokens_out, int32_t* n_tokens_out,
               int max_tokens, float* sum_logprob_out /* [batch] or NULL */);

/* the same loop, with everything whisper.cpp's per-window bookkeeping needs: the log-probability of
 * every sampled token - whisper.cpp's avg_logprobs sums the end-of-text token's too: it is slot n_tokens[b] when
 * ended_by_eot[b] - and the no-speech probability of the window (soft-max of the first, unfiltered logits row at the
 * no-speech token).  Every pointer except tokens / n_tokens may be NULL. */
typedef struct {
  int32_t* tokens;        /* [batch][max_tokens] */
  int32_t* n_tokens;      /* [batch] */
  float* sum_logprob;     /* [batch]: sum over the stored tokens (end-of-text excluded) */
  float* token_logprobs;  /* [batch][max_tokens + 1] */
  int32_t* ended_by_eot;  /* [batch]: 1 = end-of-text was sampled, 0 = a length limit stopped the window */
  float* no_speech_prob;  /* [batch] */
} ohw_greedy_result;
int ohw_greedy_ex(ohw_state* st, const ohw_sample_params* p, int batch, int max_tokens, const ohw_greedy_result* out);
/* one pass of the temperature fallback on the device, shaped like ohw_greedy_ex on the resident cross K/V: the prompt, then
 * replayed {decoder step, temperature sampler} steps.  Per row the sampler is ohw_sample_host at `temperature` (> 0): the
 * state's logit bias added, divided by the temperature, the same filter, then the first index whose partial sum of
 * probabilities reaches u * their total, u = uniforms[b][step] (ohw_rng_uniforms).  Rows with active[b] == 0 are not
 * decoded (their results are 0).  A row stops at end-of-text or a length limit only (at most max_tokens draws): the
 * caller cuts the pass at whisper.cpp's other loop exits and discards the draws it kept (ohw_rng_discard_draws).    */
int ohw_sample_pass(ohw_state* st, const ohw_sample_params* p, int batch, int max_tokens, float temperature, const int32_t* active,
                    const double* uniforms /* [batch][max_tokens] */, const ohw_greedy_result* out);
/* the same pass with best_of (1..5) candidates per window: row w * best_of + j of `out` is candidate j of window w, drawing
 * with uniforms[w][j][step]; needs max_batch >= n_windows * best_of.  The prefill and the task prompt run once per window; the
 * best_of rows of a window share that past through a kv_slot table built on the device (positions below the window's shared
 * length read the window's cache row - row w, or row w * best_of under a context table with more than one window - every
 * later position the candidate's own row; ohw_state_fetch "sample_slots" returns the table of the last call as
 * [n_windows * best_of][n_text_ctx]) and its cross K/V, streamed once per step for all of them (cross_attn_rows_kernel).  On
 * the first step every row of a window reads the window's prompt logits, so the no-speech probability is the window's and
 * is reported in each of its rows.  Windows with active[w] == 0 are not decoded (their rows' results are 0).  A row stops at
 * end-of-text or a length limit only; the step is skipped for a window once all its rows have stopped.  Language tables,
 * per-window audio contexts, context tables, the logit bias, ohw_state_set_batch_invariant and the persistent step (at most
 * 16 rows) all apply as they do to ohw_beam_search; nothing of the group layout outlives the call.  A row's arithmetic is
 * ohw_sample_pass's sampler; its decoder step takes the beam rows' kernels, so bit equality with ohw_sample_pass is not
 * promised.  best_of = 1 is ohw_sample_pass.                                                                            */
int ohw_sample_pass_n(ohw_state* st, const ohw_sample_params* p, int n_windows, int best_of, int max_tokens, float temperature,
                      const int32_t* active /* [n_windows] */, const double* uniforms /* [n_windows][best_of][max_tokens] */,
                      const ohw_greedy_result* out /* rows [n_windows * best_of] */);

/* beam search for the windows of the last ohw_encode (BASELINE.json config #5: beam = 5, hipGraph-captured decoder step).
 * The reference never uses one (Greedy{best_of:1}, src/engine/whisper.rs:243); the rule is the published Whisper
 * BeamSearchDecoder: every live beam proposes its beam_size + 1 most likely next tokens after the same logits filter, a
 * window's candidates are ranked by cumulative log-probability, sequences ending in end-of-text go to its finished pool
 * (at most beam_size), the best beam_size others become the new beams; the result is the candidate with the best
 * cumulative log-probability per token.  Device-resident like ohw_greedy: beam j of window w is decoder row w * K + j, the
 * K rows of a window stream its cross K/V once and share their common past through a slot table (no K/V copies); one
 * iteration {decoder step, top-k, update} is captured as a hipGraph and replayed.  Needs max_batch >= n_windows * beam_size. */
typedef struct {
  int32_t* tokens;      /* [n_windows][max_tokens] the best sequence, end-of-text not stored */
  int32_t* n_tokens;    /* [n_windows] */
  float* sum_logprob;   /* [n_windows] or NULL: its cumulative log-probability (end-of-text's included when it ended so) */
  int32_t* n_finished;  /* [n_windows] or NULL: sequences that reached end-of-text */
} ohw_beam_result;
int ohw_beam_search(ohw_state* st, const ohw_sample_params* p, int n_windows, int beam_size, int max_tokens, const ohw_beam_result* out);

/* the same search with what a decode policy needs to judge the result (the engine's beam pass: ohw_engine_set_beam_size).  The
 * search is ohw_beam_search's, step for step: tokens, n_tokens, sum_logprob and n_finished are the same bits.  On top of it
 * every beam carries the log-probability of each of its tokens (gathered with the token history when beams are reordered),
 * the first step also computes the window's no-speech probability from the unfiltered prompt row (bias added, no mask: what
 * ohw_greedy_ex reports), and the final ranking - the pool's sequences, topped up with the live beams by descending sum until
 * there are beam_size; best sum / max(1, n) in fp32, the first maximum - runs on the device, so only n_windows rows are
 * read back.  token_logprobs: the winner's per-token values; when it ended with end-of-text (ended_by_eot = 1: it came from
 * the finished pool) that token's value follows at index n_tokens.  Every field but tokens and n_tokens may be NULL.
 * The captured step graphs of this form are cached apart from ohw_beam_search's (they bake other pointers in).            */
typedef struct {
  int32_t* tokens;         /* [n_windows][max_tokens] */
  int32_t* n_tokens;       /* [n_windows] */
  float* sum_logprob;      /* [n_windows] or NULL */
  int32_t* n_finished;     /* [n_windows] or NULL */
  float* token_logprobs;   /* [n_windows][max_tokens + 1] or NULL */
  int32_t* ended_by_eot;   /* [n_windows] or NULL */
  float* no_speech_prob;   /* [n_windows] or NULL */
} ohw_beam_result_ex;
int ohw_beam_search_ex(ohw_state* st, const ohw_sample_params* p, int n_windows, int beam_size, int max_tokens, const ohw_beam_result_ex* out);

/* additive bias on every logits row before the filter, bias[n_vocab] (host; copied), NULL clears it.  This is the
 * engine's form of whisper.cpp's logits_filter_callback (whisper_full_params; the reference sets none,
 * src/engine/whisper.rs:243-263, so the default is no bias); tests use it to make end-of-text and timestamps win.
 * Set on ohw_engine_state(e) it holds for every state ohw_engine_transcribe decodes on (the schedules' lane states too).
 * An entry of -INFINITY is allowed and means "never": the token has probability 0 in every sampler (arg-max, draw, beam
 * candidates), counts in no log-sum-exp, the no-speech probability's included, and is never returned while another token is
 * allowed.  +INFINITY and NaN are refused (OHW_E_INVALID_ARG; the bias in effect stays).                                  */
int ohw_state_set_logit_bias(ohw_state* st, const float* bias, int n);

/* hot phrases: a history-dependent logit boost (shallow-fusion biasing), applied on the device ahead of every sampler of every
 * decoder.  whisper.cpp has no such option and the reference replaces strings in the finished transcript; the rule below is
 * this project's definition.  Off by default: with no table set, every token, log-probability, counter
 * and captured graph is what it is without the feature.
 *   A phrase is 1..OHW_PHRASE_MAX_LEN text token ids (each in [0, eot)) with a finite fp32 boost in logit units; a table holds at
 *   most OHW_PHRASE_MAX_PHRASES phrases: phrase i is tokens[offsets[i] .. offsets[i + 1]) with boosts[i] (offsets [n_phrases + 1]).
 *   The table is compiled into a trie.  Only prefixes that have a continuation are nodes.  A node has a depth d in 0..15, a path
 *   of d tokens and children (token, boost), sorted by token and unique within the node; an edge's boost is the maximum over the
 *   phrases that pass through it.  Nodes are ordered by depth, then by path, lexicographically.  The root (depth 0) holds the
 *   first tokens of all phrases.
 *   Per live row and step, before the sampler sees the row: h = the row's own sampled tokens so far, tokens[0 .. n_cur) - no
 *   prefilled context, no sot prompt; for a beam row, that beam's history in this step's view.  A node matches when d <= n_cur
 *   and the last d entries of h equal its path (at most one node per depth).  For the matching nodes in table order and for each
 *   child in token order, logit[token] = fl32(logit[token] + boost): nested matches add, and the result is reproducible to the bit.
 *   A timestamp token in the history breaks a match (no path holds one); the root always matches, so first tokens are raised at
 *   every step; there is no back-off: a boost spent on a prefix that is then abandoned is not taken back.  The row is changed in
 *   place ahead of the filter, so the boost behaves like ohw_state_set_logit_bias's: it is applied before the division by T and is
 *   inside sum_logprob, token_logprobs, the acceptance thresholds, beam scores and the first step's no-speech probability;
 *   ohw_state_fetch("logits") returns the boosted row while a table is set.  Language detection reads raw rows.  The ohw_dbg_sample*
 *   and ohw_dbg_beam_step* entries run a sampler alone, not a step: they apply no table.
 * ohw_phrase_table: the flat trie.  The caller owns the four arrays, sized for the limits (OHW_PHRASE_MAX_NODES + 1 offsets,
 *   OHW_PHRASE_MAX_PATH path tokens, OHW_PHRASE_MAX_EDGES children).  Nodes of depth d are depth_start[d] .. depth_start[d + 1] - 1;
 *   the path of node n of depth d is path[path_base[d] + (n - depth_start[d]) * d ..+ d); its children are entries child_off[n] ..
 *   child_off[n + 1] - 1 of child_tok / child_boost.
 * ohw_phrase_table_build_host: compiles the table on the host, no device needed.  OHW_E_INVALID_ARG, the phrase named, for a
 *   length of 0 or above 16, an id outside [0, eot), a non-finite boost; and for more than 1024 phrases.  n_phrases = 0 gives
 *   the empty table (no nodes).
 * ohw_phrase_boost_host: the rule on one row on the host: history [>= n_cur], row [n_vocab] changed in place.
 * ohw_state_set_phrase_table: compiles the table (eot = the model's) and sets it on the state for every later ohw_greedy*,
 *   ohw_sample_pass, ohw_sample_pass_n and ohw_beam_search* call; n_phrases = 0 clears it.  The device copy is a fixed set of
 *   buffers sized for the limits (about 0.7 MB), allocated on the first set: swapping tables captures no graph again, while "a
 *   table is set" is part of the step-graph keys.  ohw_state_phrase_count: phrases of the table in effect (0: none).
 * ohw_dbg_phrase_boost: test entry, the kernel once on caller data: logits [rows][ld] (host; read and written back whole, so a
 *   test sees every word the kernel may have touched, guard columns and guard rows included), histories [rows][max_tokens],
 *   n_cur [rows] in 0..max_tokens, done [rows], a table; n_vocab <= ld and every child token below n_vocab are checked first.
 *   The state's own table, if any, is in effect again afterwards.
 * ohw_engine_set_hot_phrases: texts[i] is tokenised with ohw_tokenize in two variants, with a leading space (the mid-sentence
 *   form) and as given (the window-start form), duplicates and forms without a token dropped (a text with no token at all:
 *   OHW_E_INVALID_ARG, the text named); boosts NULL = 1.0 each; n = 0 clears.  ohw_tokenize is a
 *   greedy longest-match and not BPE merging, so it may split a word otherwise than the model's own tokenizer would:
 *   ohw_engine_set_hot_phrases_tokens (phrase i = tokens[offsets[i] .. offsets[i + 1])) is the exact form.  The engine sets the
 *   table on its own, pipeline and lane states, states made later included, and its host-sampled ladder applies the same rule.
 *   ohw_pool_set_hot_phrases: the text form on every engine of the pool.                                                      */
#define OHW_PHRASE_MAX_LEN 16
#define OHW_PHRASE_MAX_PHRASES 1024
#define OHW_PHRASE_MAX_NODES (1 + OHW_PHRASE_MAX_PHRASES * (OHW_PHRASE_MAX_LEN - 1))
#define OHW_PHRASE_MAX_EDGES (OHW_PHRASE_MAX_PHRASES * OHW_PHRASE_MAX_LEN)
#define OHW_PHRASE_MAX_PATH (OHW_PHRASE_MAX_PHRASES * (OHW_PHRASE_MAX_LEN - 1) * OHW_PHRASE_MAX_LEN / 2)
typedef struct {
  int32_t n_phrases, n_nodes, n_edges, n_path;
  int32_t depth_start[OHW_PHRASE_MAX_LEN + 1];
  int32_t path_base[OHW_PHRASE_MAX_LEN];
  int32_t* child_off;   /* [OHW_PHRASE_MAX_NODES + 1] */
  int32_t* path;        /* [OHW_PHRASE_MAX_PATH] */
  int32_t* child_tok;   /* [OHW_PHRASE_MAX_EDGES] */
  float* child_boost;   /* [OHW_PHRASE_MAX_EDGES] */
} ohw_phrase_table;
int ohw_phrase_table_build_host(const int32_t* tokens, const int32_t* offsets, const float* boosts, int n_phrases, int eot,
                                ohw_phrase_table* out);
int ohw_phrase_boost_host(const ohw_phrase_table* table, const int32_t* history, int n_cur, float* row, int n_vocab);
int ohw_state_set_phrase_table(ohw_state* st, const int32_t* tokens, const int32_t* offsets, const float* boosts, int n_phrases);
int ohw_state_phrase_count(const ohw_state* st);
int ohw_dbg_phrase_boost(ohw_state* st, float* logits, int rows, int64_t ld, int n_vocab, const int32_t* histories, int max_tokens,
                         const int32_t* n_cur, const int32_t* done, const ohw_phrase_table* table);

/* repetition penalty and no-repeat n-grams: the two decode-time controls of faster-whisper / CTranslate2 (repetition_penalty,
 * no_repeat_ngram_size) that keep a repetition loop from forming, applied on the device ahead of every sampler of every
 * decoder.  whisper.cpp has neither.  The rule is that of transformers' RepetitionPenaltyLogitsProcessor and
 * NoRepeatNGramLogitsProcessor, restricted to text tokens.
 *   Two parameters per state: penalty theta (fp32) and ngram n (int).  Off is theta = 1.0 and n = 0, the default: nothing is
 *   launched then, and every token, log-probability, counter and captured graph is what it is without the feature.  The
 *   setter accepts OHW_REPEAT_PENALTY_MIN <= theta <= OHW_REPEAT_PENALTY_MAX and 0 <= n <= OHW_REPEAT_MAX_NGRAM, so no product
 *   leaves fp32's range; anything else, NaN included, is OHW_E_INVALID_ARG.
 *   Per live row and step, before the sampler sees the row - after the hot-phrase boost, ahead of the static bias and the filter,
 *   both of which the samplers apply themselves.  h = the row's own sampled tokens so far, tokens[0 .. n_cur), exactly the history
 *   hot phrases use: no prefilled context, no sot prompt; for a beam row, that beam's history in this step's view.
 *   1. Penalty, if theta != 1.0: for every distinct text token t (t < eot) that occurs in h, once however often it occurs,
 *      logit[t] = x < 0 ? fl32(x * theta) : fl32(x / theta), x the value after the phrase boost.  Timestamp tokens in h are not
 *      penalised: a segment legitimately ends and the next begins on the same timestamp.  With theta = 1.0 the step is skipped
 *      and no word is rewritten.
 *   2. Ban, if n >= 1 and n_cur >= n - 1: the tail is the last n - 1 entries of h (empty for n = 1).  For every start i with
 *      0 <= i <= n_cur - n and h[i .. i + n - 2] == tail (raw ids; timestamps take part like any token): if the follower
 *      f = h[i + n - 1] is a text token, logit[f] = OHW_REPEAT_BAN.  The ban comes after the penalty, so a banned token stays
 *      banned.  The constant is finite on purpose: the samplers' online log-sum-exp computes expf(v - m) with m = -inf for a
 *      thread's first element, and -inf - -inf would poison the row; -1e30 survives the bias add and the division by T >= 0.2 and
 *      underflows to probability 0.  Only text tokens are ever banned - end-of-text and timestamps never - so a row can always
 *      finish.
 *   Consequences: the modified value is inside sum_logprob, token_logprobs, the acceptance thresholds, best-of ranking and beam
 *   scores; ohw_state_fetch("logits") returns the modified rows while the rule is on.  The first step is never touched (its
 *   history is empty), so the no-speech probability is unchanged.  Language detection, ohw_state_align and the ohw_dbg_sample* /
 *   ohw_dbg_beam_step* entries are untouched; the persistent step ends at the logits and needs nothing.
 * ohw_repeat_rule_host: the rule on one row on the host, no device: history [>= n_cur], row [n_vocab] changed in place; history
 *   entries outside [0, n_vocab) are compared like any id and never written.
 * ohw_state_set_repeat_rule / ohw_state_repeat_rule: set and read a state's values, for every later ohw_greedy*, ohw_sample_pass,
 *   ohw_sample_pass_n and ohw_beam_search* call.  The values live in a two-word device buffer made at the first set: "the rule
 *   is on" is part of the step-graph keys, and a change between two settings that are both on captures nothing again.
 * ohw_dbg_repeat_rule: test entry, the kernel once on caller data: logits [rows][ld] (host; read and written back whole, guard
 *   columns and guard rows included), histories [n_entries * group][max_tokens], n_cur (or null: every history is empty) and done
 *   [n_entries].  Launch row r changes logits row r with the history of row h = r * row_mul under n_cur / done [h / group]
 *   (greedy, temperature and group passes: row_mul = group = 1; beam search: group = K, its first step row_mul = K).  Checked
 *   before the launch: shapes, n_vocab <= ld, 0 <= eot, every n_cur in 0..max_tokens, (rows - 1) * row_mul / group < n_entries,
 *   penalty and ngram as the setter checks them.  The state's own setting is in effect again afterwards.
 * ohw_engine_set_repetition: the values on the engine's own state and its pipeline and lane states, states made later included;
 *   its host-sampled ladder applies ohw_repeat_rule_host right behind ohw_phrase_boost_host.  ohw_pool_set_repetition: the same
 *   on every engine of the pool.                                                                                              */
#define OHW_REPEAT_BAN (-1.0e30f)
#define OHW_REPEAT_PENALTY_MIN 0.01f
#define OHW_REPEAT_PENALTY_MAX 100.0f
#define OHW_REPEAT_MAX_NGRAM 32
int ohw_repeat_rule_host(float penalty, int ngram, const int32_t* history, int n_cur, float* row, int n_vocab, int eot);
int ohw_state_set_repeat_rule(ohw_state* st, float penalty, int ngram);
int ohw_state_repeat_rule(const ohw_state* st, float* penalty, int* ngram);
int ohw_dbg_repeat_rule(ohw_state* st, float* logits, int rows, int64_t ld, int n_vocab, const int32_t* histories, int max_tokens,
                        const int32_t* n_cur, const int32_t* done, int n_entries, int row_mul, int group, float penalty, int ngram,
                        int eot);

/* command lists: constrain a window to a closed list of phrases, on the device ahead of every sampler of every decoder.
 * whisper.cpp does this with grammar / grammar_penalty in whisper_full_params and its `command` example: rejected text tokens
 * are lowered by grammar_penalty (default 100), and end-of-text too while the grammar cannot accept - recalled from upstream,
 * unpinned.  A phrase list is the finite special case of that grammar; the rule below is this project's definition of it
 * (DESIGN.md section 9).  Off by default: with no list set nothing is launched, and every token, log-probability, counter and
 * captured graph is what it is without the feature.
 *   A list is 1..OHW_PHRASE_MAX_PHRASES phrases of 1..OHW_PHRASE_MAX_LEN text token ids (each in [0, eot)); phrase i is
 *   tokens[offsets[i] .. offsets[i + 1]); duplicates are allowed.  It compiles into an ANCHORED trie, ohw_command_table: every
 *   prefix of every phrase is a node, the empty prefix (the root, depth 0) and the full phrases (up to depth 16) included.  Nodes
 *   are ordered by depth, then by path, lexicographically, as in ohw_phrase_table; the path of node n of depth d is
 *   path[path_base[d] + (n - depth_start[d]) * d ..+ d), its children are child_tok[child_off[n] .. child_off[n + 1]), sorted and
 *   unique; terminal[n] = 1 when some phrase ends at n, and phrase_id[n] = the lowest index of such a phrase, else -1.
 *   Per live row and step, behind the hot-phrase boost and the repetition rule and ahead of the sampler (which adds the static
 *   bias and runs its own filter afterwards): h = the row's own sampled tokens tokens[0 .. n_cur), the history the other two rules
 *   use (no prompt, no prefilled context; a beam row: that beam's view); nothing at or behind tokens[n_cur] is read.  t = the
 *   entries of h in [0, eot), in order: timestamps and other specials are skipped, so a leading <|0.00|> breaks no match.
 *   d = len(t).  The row's node is the depth-d node whose path equals t; with d > 16 or no such node the row is OFF THE LIST.
 *   With penalty p:
 *     text tokens   every column < eot that is not a child of the row's node becomes fl32(x - p), with p = +inf OHW_REPEAT_BAN
 *                   (finite, for the reason given there); children are not touched; off the list every text column is lowered
 *     end-of-text   lowered the same way, unless the node is terminal or the row is off the list: then it is not touched
 *     >= eot + 1    timestamps and every other id: never touched
 *   Each word is read once and written at most once; words the rule leaves alone are not rewritten.  The host twin does the same
 *   single fp32 subtraction, so the two agree to the bit.  0 < p <= OHW_COMMAND_PENALTY_MAX or p = +inf; NaN, zero and negatives
 *   are OHW_E_INVALID_ARG.
 *   List probability: at a step with d == 0 the first decoder row of each window also writes list_logprob[window] =
 *   LSE(x over the root's children) - LSE(x over all columns < eot), in fp32 on the row as the kernel finds it, before lowering:
 *   given that text comes next, the probability that the unconstrained model starts a listed phrase - the handle for rejecting
 *   off-list speech, like the first step's no-speech probability.  The latest such step wins (with timestamps, usually the step
 *   behind the opening timestamp).  -inf logits mean "never" and enter neither sum; all children at -inf give -inf, not NaN.
 *   Rows with d == 0 of a window's first decoder row are read a second time for this (the maxima first, then the sums).
 *   Consequences: the lowered row is inside sum_logprob, token_logprobs, the acceptance thresholds, best-of ranking, beam scores
 *   and the first step's no-speech probability, as the boost is: under a hard list a silent window can pass the no-speech rule;
 *   list_logprob and the speech detector are the remedies.  ohw_state_fetch("logits") returns lowered rows while a list is set.
 *   Language detection, ohw_state_align, prefill, the persistent step and the ohw_dbg_sample* / ohw_dbg_beam_step* entries are
 *   untouched.  A row can always finish: a node that is not terminal has a child, terminal and off-list rows keep end-of-text,
 *   timestamps are never touched.  The sampler's own filter (suppress_blank, timestamp pairing) still applies afterwards: a
 *   phrase whose first token is the model's blank token cannot start a window.
 * ohw_command_table: the caller owns the five arrays, sized for the limits.  ohw_command_table_build_host: compiles a list on the
 *   host, no device; the refusals of ohw_phrase_table_build_host, the phrase named; n_phrases = 0 gives the empty table.
 * ohw_command_rule_host: the rule on one row on the host: history [>= n_cur], row [n_vocab] changed in place; *list_logprob_out
 *   (may be null) is written only when d == 0, summed in double.  ohw_command_match_host: phrase_id of the node whose path equals
 *   the entries of tokens[0 .. n) below the table's eot, when it is terminal; else -1.
 * ohw_state_set_command_table: compiles the list (eot = the model's) and sets it with the penalty for every later ohw_greedy*,
 *   ohw_sample_pass, ohw_sample_pass_n and ohw_beam_search* call; n_phrases = 0 clears it.  The device copy is one buffer sized
 *   for the limits (about 0.8 MB) holding the penalty too, made at the first set: "a list is set" is part of the step-graph keys,
 *   and swapping lists or penalties captures nothing again.  ohw_state_command_count: phrases of the list in effect (0: none).
 * ohw_state_command_list_logprob: out[0 .. batch) = list_logprob of the windows of the last decoding call on this state.  An entry
 *   is written by its window's d == 0 steps only: a window that was done when the call began keeps its earlier value, and before
 *   any such step an entry is NaN.  OHW_E_INVALID_ARG with no list set or batch outside 1..max_batch.
 * ohw_dbg_command_rule: test entry, the kernel once on caller data, the arguments and checks of ohw_dbg_repeat_rule: logits
 *   [rows][ld] come back whole (guard rows and columns included), list_logprob [n_entries] is read and written back whole (fill
 *   it with a sentinel), row h writes it when h % group == 0.  The state's own list is in effect again afterwards.
 * ohw_engine_set_commands: the text form.  texts[i] is tokenised with ohw_tokenize as given and with a leading space; both forms
 *   belong to index i (a form without a token, or equal to the other, is dropped; a text with no token at all:
 *   OHW_E_INVALID_ARG, the text named).  ohw_tokenize is a greedy longest-match and not BPE merging, so it may split a word
 *   otherwise than the model's tokenizer would: ohw_engine_set_commands_tokens is the exact form.  n = 0 clears.  The engine sets
 *   the list on its own, pipeline and lane states, states made later included; its host-sampled ladder applies
 *   ohw_command_rule_host right behind ohw_repeat_rule_host.  ohw_pool_set_commands: the text form on every engine of the pool.
 * ohw_engine_last_commands: one ohw_command_hit per kept window of the last transcribe call (of recording i of a batch call, in
 *   window order, `window` counted within the recording): phrase = the caller's index when the kept tokens' text tokens equal a
 *   listed phrase exactly, else -1; list_logprob belongs to the kept pass, device and host ladders alike.  Empty with no list.  */
#define OHW_COMMAND_PENALTY_MAX 1000.0f
#define OHW_COMMAND_PENALTY_DEFAULT 100.0f
#define OHW_COMMAND_MAX_NODES (1 + OHW_PHRASE_MAX_PHRASES * OHW_PHRASE_MAX_LEN)
#define OHW_COMMAND_MAX_EDGES (OHW_PHRASE_MAX_PHRASES * OHW_PHRASE_MAX_LEN)
#define OHW_COMMAND_MAX_PATH (OHW_PHRASE_MAX_PHRASES * OHW_PHRASE_MAX_LEN * (OHW_PHRASE_MAX_LEN + 1) / 2)
typedef struct {
  int32_t n_phrases, n_nodes, n_edges, n_path, eot;
  int32_t depth_start[OHW_PHRASE_MAX_LEN + 2];
  int32_t path_base[OHW_PHRASE_MAX_LEN + 1];
  int32_t* child_off;   /* [OHW_COMMAND_MAX_NODES + 1] */
  int32_t* path;        /* [OHW_COMMAND_MAX_PATH] */
  int32_t* child_tok;   /* [OHW_COMMAND_MAX_EDGES] */
  int32_t* terminal;    /* [OHW_COMMAND_MAX_NODES] */
  int32_t* phrase_id;   /* [OHW_COMMAND_MAX_NODES] */
} ohw_command_table;
typedef struct { int32_t window, phrase; float list_logprob; } ohw_command_hit;
int ohw_command_table_build_host(const int32_t* tokens, const int32_t* offsets, int n_phrases, int eot, ohw_command_table* out);
int ohw_command_rule_host(const ohw_command_table* table, float penalty, const int32_t* history, int n_cur, float* row, int n_vocab,
                          int eot, float* list_logprob_out);
int ohw_command_match_host(const ohw_command_table* table, const int32_t* tokens, int n);
int ohw_state_set_command_table(ohw_state* st, const int32_t* tokens, const int32_t* offsets, int n_phrases, float penalty);
int ohw_state_command_count(const ohw_state* st);
int ohw_state_command_list_logprob(ohw_state* st, int batch, float* out);
int ohw_dbg_command_rule(ohw_state* st, float* logits, int rows, int64_t ld, int n_vocab, const int32_t* histories, int max_tokens,
                         const int32_t* n_cur, const int32_t* done, int n_entries, int row_mul, int group, float penalty, int eot,
                         const ohw_command_table* table, float* list_logprob);

/* the persistent small-batch decoder step (default OFF; OHW_DEC_PERSIST=1 turns it on for new states): single-token steps
 * of at most 16 rows - one utterance, the K rows of a beam search - run their 32 layers as ONE launch whose workgroups hand
 * activations to each other (openhush_amd/csrc/decode_persist.hip) instead of 8 launches per layer.  Correct (tests/
 * test_gpu_persist.py) and slower than the launches on MI355X: every all-to-all hand-off between the 256 workgroups costs
 * 3 - 6.5 us against 1.6 us of kernel boundary + 1.9 us of first-byte latency (profiles/r03_persist_trace.txt; large-v3,
 * one row: 2.2 ms per token against 1.44).  Never used under ohw_state_set_batch_invariant.  Results are deterministic and
 * a row's result does not depend on the other rows.                                                                        */
int ohw_state_set_persistent(ohw_state* st, int on);

/* batch-invariant decoding (default off): the decoder picks some kernel variants from the number of rows in flight - up to
 * 24 rows the keys of a cross-attention (row, head) are cut over several workgroups, and the prompt pass shares one K/V
 * stream among a window's rows only when there are enough windows - and a different variant sums the softmax in a
 * different order (last-bit differences in the logits).  With this on, the variant depends on n_new alone, so a window's
 * logits and tokens are bit-identical whatever batch it is decoded in; tiny batches lose a little latency.
 * ohw_engine_transcribe turns it on for audio longer than one batch, which makes its schedules agree token for token. */
int ohw_state_set_batch_invariant(ohw_state* st, int on);

/* reduced audio context (whisper.cpp's whisper_full_params.audio_ctx, whisper-rs set_audio_ctx; the reference sets none,
 * so the default is the full context).  With n_ctx = C, 1 <= C <= n_audio_ctx: conv1 sees mel frames 0 .. 2C-1 of the
 * window with zero padding on both sides (frame 2C is padding, not audio), conv2 produces C rows and adds positional rows
 * 0 .. C-1, the encoder and the cross-K/V projection run on C positions per window, cross K/V are stored packed
 * [2L][B][H][C][64], and every decoder cross-attention reads C keys: encoder work, cross-K/V bytes and cross-attention
 * bytes scale with the audio, not with the 30 s window.  The log-mel spectrogram (its clamp maximum too) does not change.
 * 0 or n_audio_ctx = full context; a value outside 0..n_audio_ctx returns OHW_E_INVALID_ARG.  The setting holds for later
 * ohw_mel*, ohw_encode*, ohw_decode*, ohw_greedy*, ohw_sample_pass, ohw_beam_search and ohw_detect_language calls; an
 * encode under another context than the last ohw_mel* of the state, or a decode under another context than its last
 * encode, returns OHW_E_INVALID_ARG (neither ever reads a stale image or stale K/V).  Buffers stay sized for n_audio_ctx. */
int ohw_state_set_audio_ctx(ohw_state* st, int n_ctx);
int ohw_state_audio_ctx(const ohw_state* st);   /* the context in effect, 1..n_audio_ctx (n_audio_ctx = full) */
/* the context that covers n_samples of 16 kHz audio (host only, no device):
 *     min(1500, round_up(ceil(n_samples / 320) + 32, 64))
 * one encoder position is 320 samples; the 32 extra positions are 0.64 s of headroom behind the last sample, and the
 * multiple of 64 matches the key block of the encoder's attention.  1.1 s -> 128, 5 s -> 320, more than 28.8 s -> 1500.     */
int32_t ohw_audio_ctx_for(int64_t n_samples);
/* per-window audio context inside one batch, for the next ohw_mel* / ohw_encode* and the decodes on them.
 * n_ctx[b], b < batch: 1 <= n_ctx[b] <= E, where E is the state's context in effect (ohw_state_audio_ctx: the "envelope").
 * NULL (or batch 0) clears it: every window runs at E.  batch must equal the batch of the ohw_mel* that follows.
 * Layouts and strides are those of a uniform run at E (activations [B][E][d], cross K/V [2L][B][H][E][64]); window b uses
 * its first n_ctx[b] rows of each: its mel image ends at frame 2 * n_ctx[b], the encoder's attention runs n_ctx[b] queries
 * against n_ctx[b] keys, every cross-attention streams n_ctx[b] keys.  Rows from n_ctx[b] on are unspecified and no valid
 * row depends on them; the valid rows carry the bits of a uniform run at ohw_state_set_audio_ctx(n_ctx[b]).  The encoder's
 * GEMMs and LayerNorms still run B * E rows unless ohw_state_set_packed_encoder is on.  The lengths live in device memory, so a captured
 * greedy / beam step graph is reused across every mix of one envelope.  While lengths are set the cross-attention variant
 * is picked as under ohw_state_set_batch_invariant (never a key-split form) and the persistent step is not used.
 * An encode under other lengths than the last ohw_mel*'s, or a decode after the lengths changed without a new encode,
 * returns OHW_E_INVALID_ARG.  ohw_encode_slice records its windows' lengths into decode-batch slots first .. first + batch - 1;
 * the slices of one decode batch run all with or all without lengths.  ohw_state_set_audio_ctx clears the lengths.       */
int ohw_state_set_window_ctx(ohw_state* st, const int32_t* n_ctx, int batch);
int ohw_state_window_ctx(const ohw_state* st, int window);   /* the context of a decode-batch slot of the last encode; E when it ran without lengths */
/* packed-row encoder (default 0; OHW_ENC_PACKED=1 turns it on for new states): an encode under per-window lengths runs the
 * encoder on the sum of the lengths instead of B * E rows.  The setting is read at encode time and has no effect without
 * lengths, or when every length equals E (that is the uniform layout: the unpacked path runs).
 * Layout, inside the encoder only: off[b] = n_ctx[0] + .. + n_ctx[b - 1], Mp = off[B]; row off[b] + t of every encoder
 * activation behind the conv stem (residual stream, LayerNorm output, q|k|v, attention output, mlp hidden, encoder output, the
 * "block0" tap) is position t of window b; rows are neither padded nor tile-aligned, and Mp <= B * E fits the buffers as they
 * are.  conv1 / conv2 and the "stem" tap keep the unpacked layout; one gather packs conv2's valid rows.  LayerNorms and dense
 * GEMMs run Mp rows, the attention finds window b at off[b], the cross-K/V projection scatters its rows back, so everything
 * behind the encoder is unchanged: cross K/V stay [2L][B][H][E][64], the decoder, its graphs and the refusals above too.
 * The valid rows of the encoder output and of the cross K/V, and every token and log-probability decoded from them, carry
 * the bits of the unpacked run.  ohw_state_fetch keeps returning [B][E][d] for "block0" / "enc" / "xk<l>" / "xv<l>" (the
 * encoder taps are unpacked on the way out; rows from n_ctx[b] on are unspecified, as without packing).  set returns
 * OHW_E_INVALID_ARG for a NULL state; the getter returns 0 / 1.                                                       */
int ohw_state_set_packed_encoder(ohw_state* st, int on);
int ohw_state_packed_encoder(const ohw_state* st);

/* per-window language inside one decode batch (opt-in; with no table every call computes what it computed before).
 * ohw_state_set_window_lang: lang_ids[b], b < batch, is a language id 0 .. n_langs - 1 ("explicit") or OHW_LANG_DETECT
 * ("pending": ohw_state_detect_window_lang resolves it); NULL (or batch 0) clears the table.  OHW_E_INVALID_ARG for an id
 * outside that range, for batch > max_batch and for an English-only model (n_vocab < 51865: its prompt has no language token).
 * The table lives in device memory; the host keeps only which entries are explicit, pending or resolved.
 * While a table is set, ohw_greedy, ohw_greedy_ex, ohw_sample_pass and ohw_beam_search ignore p->lang_id: a device kernel
 * writes window b's prompt row with sot + 1 + table[b] (all beams of a window share it), so detected ids never reach the
 * host.  The table's batch must equal the decode batch (for ohw_encode_slice: total), and a decode with a pending entry
 * returns OHW_E_INVALID_ARG - it never silently becomes English.  The prompt is outside the replayed step graphs and the
 * sampler parameters do not change, so decoding again with other languages captures nothing.
 * ohw_state_detect_window_lang: for the windows of the last encode, one decoder step on [sot] at position 0 (the step of
 * ohw_detect_language; it runs under audio_ctx, per-window lengths and the packed encoder as they stand), then the pick on
 * the state's logits buffer: arg-max over the raw language columns (no logit bias, no filter), the lowest id on ties, and an
 * fp32 soft-max over those columns.  Only pending entries are resolved; explicit ones are kept.  No logits leave the device.
 * ohw_state_window_lang: ids_out [batch] (OHW_LANG_DETECT for an entry still pending); probs_out [batch][n_langs] or NULL:
 * the soft-max of a resolved row, 1 at the id of an explicit row, zeros for a pending row.
 * Every ohw_encode* turns resolved entries back into pending (they belonged to the old audio); explicit entries persist.
 * ohw_state_set_audio_ctx and ohw_state_set_window_ctx do not touch the table.                                          */
enum { OHW_LANG_DETECT = -1 };
int ohw_state_set_window_lang(ohw_state* st, const int32_t* lang_ids, int batch);
int ohw_state_detect_window_lang(ohw_state* st, int batch);
int ohw_state_window_lang(ohw_state* st, int batch, int32_t* ids_out, float* probs_out);
/* per-window text context ("prompted decoding"; opt-in: with no table every call computes what it computed before).
 * ohw_state_set_window_prompt: tokens [batch][stride], n_tokens [batch]: decode-batch slot b decodes behind n_tokens[b] context
 * tokens - text so far: an initial prompt, or the text of the chunk before - with ids in 0 .. n_vocab - 1 and
 * 0 <= n_tokens[b] <= n_text_ctx / 2 - 1 (OHW_E_INVALID_ARG otherwise, and for batch > max_batch); tokens NULL (or batch 0) clears
 * the table.  A slot with n_tokens[b] = 0 has no context and gets no [prev] token; a slot with n > 0 occupies n + 1 positions:
 * [prev], then its tokens.  The table is uploaded once and lives in device memory.
 * ohw_state_window_prompt_len: the positions slot `window`'s context occupies, 0 or n + 1.
 * ohw_state_prefill: for the windows of the last encode (batch must equal its batch and the table's; active [batch] or NULL: the
 * windows to serve), runs the context through the decoder in chunks of 8 positions at n_past = 0, 8, .. and leaves every
 * layer's self K/V of positions 0 .. len[b] - 1 in cache row b; no logits.  A window whose context ends inside a chunk is fed
 * [eot] in the surplus rows: they write cache positions at or past len[b], which a decode that starts at n_past = len[b]
 * overwrites before it reads them.  Windows a chunk has nothing for are skipped by its cross-attention.  A no-op while no table
 * is set.  Callers of ohw_decode / ohw_decode_active call it themselves and start at n_past = len[b].
 * While a table is set, ohw_greedy, ohw_greedy_ex, ohw_sample_pass (for its active windows) and ohw_beam_search run the prefill
 * first and start window b at position len[b]; n_max is capped by n_text_ctx - n_prompt - the largest len.  The context is not
 * part of the returned tokens, log-probabilities or counts, and the timestamp and blank rules see the window's own tokens only.
 * ohw_beam_search keeps window w's context and prompt in cache row w * beam_size, which only w's beams write.
 * Positions are device data: decoding again under other lengths captures no graph, as long as p->n_max does not exceed the cap
 * above (the capped value is one of the sampler parameters a captured step is keyed by; the default n_max never exceeds it).  ohw_state_align replays without the context.
 * OHW_PREFILL_XA=0 (read when a state is created) sends the chunks' cross-attention through the single-row kernels (an A/B knob). */
int ohw_state_set_window_prompt(ohw_state* st, const int32_t* tokens, int stride, const int32_t* n_tokens, int batch);
int ohw_state_window_prompt_len(const ohw_state* st, int window);
int ohw_state_prefill(ohw_state* st, int batch, const int32_t* active);
/* the prefill's chunk size: 8 (default) or 16 positions per pass (anything else: OHW_E_INVALID_ARG).  With 16 a prefill makes half
 * as many passes, so the decoder weights and every window's cross K/V are streamed half as often, and its cross-attention fills
 * all 16 columns of its MFMA tile (cross_attn_chunk_kernel<T, 16, VAR>).  Surplus rows of a chunk then reach cache positions up to
 * len[b] + 15, still inside n_text_ctx and still overwritten by the decode before a query reads them.  A table that is set is laid
 * out again for the new size; the results agree with chunk 8 within the decoder's rounding (the GEMMs see other row counts), not
 * bit for bit.  ohw_decode / ohw_decode_active keep their limit of 8 tokens per window, ohw_state_align replays in chunks of 8.
 * ohw_state_prefill_chunk reads the setting back.  ohw_engine_set_prefill_chunk: the setting on the engine's own, pipeline and
 * lane states, those made later included.                                                                                    */
int ohw_state_set_prefill_chunk(ohw_state* st, int positions);
int ohw_state_prefill_chunk(const ohw_state* st);
/* text -> token ids, the scheme of whisper.cpp's tokenizer restated (csrc/tokenize.cpp states the rule): the text is split into
 * pieces (contractions; an optional space and a run of letters, of digits, or of other non-space bytes; runs of white space), and
 * inside a piece the longest vocabulary entry that is a prefix of the rest is taken, again and again; a byte no entry starts
 * with is skipped.  Both return the number of tokens written to out [cap], or OHW_E_INVALID_ARG when cap is too small.
 * ohw_tokenize_host: the vocabulary is n_vocab entries laid end to end in vocab_bytes, entry i of lens[i] bytes and id i.
 * ohw_tokenize: the model's text tokens (ids below end-of-text).  No device needed.
 * ohw_prompt_clip_host: a prompt keeps its LAST n_text_ctx / 2 - 1 tokens; out [min(n, n_text_ctx / 2 - 1)]; returns the count. */
int ohw_tokenize_host(const char* vocab_bytes, const int32_t* lens, int n_vocab, const char* text, int32_t* out, int cap);
int ohw_tokenize(const ohw_ctx* ctx, const char* text, int32_t* out, int cap);
int ohw_prompt_clip_host(const int32_t* in, int n, int n_text_ctx, int32_t* out);
/* what the device pick computes, on the host: row is one logits row [n_vocab]; *id = arg-max of row[sot + 1 + i], i < n_langs
 * (the first maximum), probs [n_langs] or NULL = soft-max over those columns in fp32 arithmetic.  No device needed.  A row
 * whose language columns are all -inf or NaN gives id 0 and NaN probabilities, on the host and on the device alike.        */
int ohw_lang_pick_host(const float* row, const ohw_special_tokens* tok, int32_t* id, float* probs);

/* ---- word timestamps: cross-attention alignment (the published openai-whisper find_alignment; whisper.cpp's
 *      dtw_token_timestamps), on the device, for windows whose cross K/V is still resident.  The reference sets no such
 *      option; its user guide lists video captions as a use, and a caption needs times.
 * ohw_state_set_align_heads: the (decoder layer, head) pairs whose cross-attention carries the alignment, at most
 *   OHW_ALIGN_MAX_HEADS; there is no built-in preset (INTEGRATION.md says where upstream lists them per checkpoint).  NULL or
 *   n = 0 clears the list and frees the buffers below.  OHW_E_INVALID_ARG for a pair outside the model (the message names its
 *   index) and for n > OHW_ALIGN_MAX_HEADS.  Until a list is set ohw_state_align returns OHW_E_INVALID_ARG.
 *   The buffers are made here, on the first list and again when the number of pairs A changes: probabilities f32
 *   [max_batch][A][n_text_ctx / 2 + 8][n_audio_ctx], the tapped queries f32 [max_batch][n_text_ctx / 2 + 8][A][64], column
 *   statistics f32 [max_batch][A][n_audio_ctx][2], m f32 [max_batch][n_text_ctx / 2 + 1][n_audio_ctx], trace bytes
 *   [max_batch][(n_text_ctx / 2 + 2) * (n_audio_ctx + 1)], indices i32 [max_batch][n_text_ctx / 2 + 1].  At large-v3 with
 *   max_batch 32 and 10 pairs: 445.4 MB + 19.0 MB + 3.8 MB + 43.2 MB + 10.9 MB + 0.03 MB = 522 MB (1.55 GB with 32 pairs).
 * ohw_state_align: for the windows of the last encode (batch = its batch).  tokens [batch][stride]: the first n_tokens[b]
 *   entries of row b are window b's text tokens (ids 0 .. eot - 1), in order; n_tokens[b] = 0 skips the window (its row of
 *   start_idx_out is left alone); n_frames[b] = the window's 10 ms frames of real audio.  start_idx_out [batch][stride + 1]:
 *   entry k < n_tokens[b] is the encoder position (20 ms each) at which text token k starts, entry n_tokens[b] the position
 *   at which the last token ends.  Time in seconds = index * 0.02 + the window's offset in the recording.
 *   The method, per window:
 *     sequence   the window's prompt as it was decoded - sot, the language token (from the per-window language table when one
 *                is set, else p->lang_id) and the task token (p->translate) on a multilingual model - then [no_timestamps],
 *                the text tokens, [eot]: N_all tokens, the first P of them the prompt with [no_timestamps];
 *     replay     the sequence is fed through the decoder in chunks of 8 tokens per window from position 0 of the state's self
 *                K/V cache (a window's tail is padded with eot: causality keeps padding from reaching real rows), always on
 *                the launch-per-kernel step, never the persistent or the fused-attention one, and without capturing a graph.
 *                AFTER THE CALL THE STATE'S SELF K/V IS STALE; every decode entry starts at position 0 and rewrites it;
 *     tap        behind the cross-query GEMM of each listed layer: p[a][i][t] = soft-max over t < n_keys of the logits
 *                (q_i * 0.125) . k_t the layer's cross-attention uses, fp32; n_keys = max(1, min(the window's audio context
 *                in effect, n_frames / 2)); keys from n_keys on have probability exactly 0 and influence nothing;
 *     reduce     per head and key column the mean and the population standard deviation over the N_all rows,
 *                z = (p - mean) / std (a column with std == 0 becomes 0), a median of width 7 along t with the edges padded as
 *                numpy.pad(mode = "reflect") pads, the mean over the heads, rows P .. N_all - 1 kept: m [N][n_keys] fp32,
 *                N = n_tokens + 1;
 *     DTW        on x = -m in fp32: cost[0][0] = 0, the rest of row 0 and column 0 +inf, cost[i][j] = x[i-1][j-1] + c with
 *                c0 = cost[i-1][j-1], c1 = cost[i-1][j], c2 = cost[i][j-1]: c0 (trace 0) if c0 < c1 && c0 < c2, else c1
 *                (trace 1) if c1 < c0 && c1 < c2, else c2 (trace 2); walked back from (N, n_keys) with trace[0][*] = 2 and
 *                trace[*][0] = 1; a row's index is the key at which the path first enters it.
 *   It honours ohw_state_set_audio_ctx, ohw_state_set_window_ctx, the packed encoder and the language table.  Refused with
 *   OHW_E_INVALID_ARG before any launch: no head list; batch other than the last encode's; a token id < 0 or >= eot (window and
 *   position named); n_tokens[b] < 0, > stride or > n_text_ctx / 2 (window named); n_frames[b] < 0; a call under another audio
 *   context or other per-window contexts than the last encode; a language table with a pending entry (window named).
 * ohw_align_reduce_host / ohw_dtw_host: the reduction and the DTW above on the host, no device needed; the device kernels
 *   run the same fp32 operations in the same order.  p [n_heads][n_all][n_keys], m_out [n_all - n_prompt][n_keys];
 *   m [n][n_keys], start_idx_out [n].
 * Cost and side effects: every chunk is a whole run_decoder_step - the layers behind the last listed one, the final LayerNorm
 *   and the logits GEMM of its 8 rows per window run too and their results are not read - and it counts in ohw_dbg_counter's
 *   "dec_gemm.*" / "xattn.*" / "self_attn.*" tallies like any other step.  An ohw_encode* ends the validity of "align_*".
 * ohw_state_fetch gains "align_q" [N_all][A][64] (the tapped query rows, scaled so that the logits are exactly q . k),
 *   "align_p" [A][N_all][n_keys] and "align_m" [N][n_keys] of window batch - 1 of the last ohw_state_align.            */
#define OHW_ALIGN_MAX_HEADS 32
typedef struct { int32_t layer, head; } ohw_align_head;
int ohw_state_set_align_heads(ohw_state* st, const ohw_align_head* heads, int n);
int ohw_state_align(ohw_state* st, const ohw_sample_params* p, const int32_t* tokens, int stride, const int32_t* n_tokens,
                    const int32_t* n_frames, int batch, int32_t* start_idx_out);
int ohw_align_reduce_host(const float* p, int n_heads, int n_all, int n_prompt, int n_keys, float* m_out);
int ohw_dtw_host(const float* m, int n, int n_keys, int32_t* start_idx_out);
/* ---- times in the engine.  ohw_engine_set_word_timestamps(e, heads, n): the alignment heads of every state the engine decodes
 *      on; NULL / 0 = off (the default).  When on, every schedule and the seek loop align the kept pass of each window on the
 *      state that decoded it, before that state's next encode (ohw_state_align; beam or ladder results alike); windows dropped
 *      by the no-speech rule or without a text token are skipped.  Tokens and text do not change.  Results of the last
 *      ohw_engine_transcribe, valid until the next call:
 *   token times  one entry per aligned text token: its id, the index of its window (as in ohw_engine_last_quality), t0 / t1 in
 *                seconds = the alignment's start / end index * 0.02 + the window's offset in the recording; empty when off;
 *   words        (needs the alignment; empty when off) a word starts at the first text token of a window, and at any token whose
 *                bytes begin with a space provided the bytes in front of it end on a complete UTF-8 sequence; t0 / t1 are those of
 *                its first / last token; punctuation is not merged.  ohw_word_starts_host is the rule: bytes = the tokens' bytes
 *                of ONE window concatenated, lens[i] = bytes of token i, starts_out[i] = 1 where a word starts;
 *   segments     (always available, no alignment needed) within a window's kept tokens the text between consecutive timestamp
 *                tokens is one segment, t0 / t1 = (ts - timestamp_begin) * 0.02 + the window's offset; text in front of the
 *                first timestamp starts at the window's offset; text with no closing timestamp ends at the earlier of the
 *                window's end and the recording's end.  ohw_segments_host is the rule on one window's tokens: it returns the
 *                number of segments (at most cap are written): tokens [first, end) of the list, t0, t1.
 *   text_off / text_len index ohw_engine_last_text (the trimmed text).  ohw_engine_batch_times: the same three arrays for
 *   recording i of the last ohw_engine_transcribe_batch (any pointer may be NULL), indexing ohw_engine_batch_result's text.
 *   Turning the setting off also frees the alignment buffers of every state of the engine.
 *   ohw_pool_set_word_timestamps: the setting on every engine of the pool; ohw_pool_transcribe gathers the three arrays in
 *   recording order next to the tokens (window = the window of the recording, offsets into ohw_pool_last_text):
 *   ohw_pool_last_token_times / _last_words / _last_segments.                                                            */
typedef struct { int32_t id, window; float t0, t1; } ohw_token_time;
typedef struct { size_t text_off, text_len; float t0, t1; } ohw_span_time;
typedef struct { int32_t first, end; float t0, t1; } ohw_token_span;
struct ohw_engine;
int ohw_engine_set_word_timestamps(struct ohw_engine* e, const ohw_align_head* heads, int n);
int ohw_engine_last_token_times(struct ohw_engine* e, const ohw_token_time** t, int* n);
int ohw_engine_last_words(struct ohw_engine* e, const ohw_span_time** w, int* n);
int ohw_engine_last_segments(struct ohw_engine* e, const ohw_span_time** s, int* n);
int ohw_engine_batch_times(struct ohw_engine* e, int i, const ohw_token_time** token_times, int* n_token_times,
                           const ohw_span_time** words, int* n_words, const ohw_span_time** segments, int* n_segments);
struct ohw_pool;
int ohw_pool_set_word_timestamps(struct ohw_pool* p, const ohw_align_head* heads, int n);
int ohw_pool_last_token_times(struct ohw_pool* p, const ohw_token_time** t, int* n);
int ohw_pool_last_words(struct ohw_pool* p, const ohw_span_time** w, int* n);
int ohw_pool_last_segments(struct ohw_pool* p, const ohw_span_time** s, int* n);
int ohw_word_starts_host(const char* bytes, const int32_t* lens, int n, int32_t* starts_out);
int ohw_segments_host(const int32_t* tokens, int n, const ohw_special_tokens* tok, float t_off, float t_end, ohw_token_span* out, int cap);

/* ---- confidence: how sure the UNCONSTRAINED model was of each token of a transcript (openai-whisper's word `probability`,
 *      whisper.cpp's per-token `p`), on the device, for windows whose cross K/V is still resident.
 * Why not the decode's own token_logprobs: those are taken behind the logit bias, the hot-phrase boost, the repetition rule, the
 *   command list and the temperature - under a hard command list every kept token has a decode log-probability near 0 whatever
 *   the audio was.  A confidence is a teacher-forced pass over the kept tokens with a soft-max over the RAW logits.
 * The sequence: for window b with n text tokens t_0 .. t_{n-1} (ids 0 .. eot - 1, timestamps already removed) it is
 *   ohw_state_align's: [sot, (lang, task), no_timestamps, t_0 .. t_{n-1}].  P = the prompt length (4 multilingual, 2 not); there
 *   is no previous-text context.  Position P - 1 + i predicts t_i for i < n, position P - 1 + n predicts end-of-text.
 * The score of a row: x = that position's raw fp32 logits (no logit bias, no rule, no temperature, no filter):
 *     logit     = x[target]                     target = t_i, or eot for row n
 *     lse_text  = log sum_{j < eot}     exp(x[j])
 *     lse_all   = log sum_{j < n_vocab} exp(x[j])
 *     top_id    = the first j < eot with x[j] == max_{j < eot} x[j];   top_logit = x[top_id]
 *   logit, top_id and top_logit are selections: the very 32-bit words the logits buffer holds.  The two lse values are fp32
 *   reductions whose shape is a function of n_vocab and eot only (score.hip states the order): a row's five words never depend on
 *   the batch, the row's place in it or the CU budget.  ohw_token_score_host is the rule on one row, no device needed.
 *   ohw_token_prob_host (any output may be NULL): openai's text-token log-probability logit - lse_text, the full-vocabulary
 *   log-probability logit - lse_all (summed over rows 0 .. n: the sequence log-likelihood, for rescoring), top_logit - lse_text.
 * Word probability: words are cut by ohw_word_starts_host on the window's text tokens; a word's probability is the arithmetic
 *   mean of exp(logit - lse_text) of its tokens (openai-whisper's timing.py), accumulated in double and rounded once to float.
 *   ohw_word_probs_host is the rule: logprob_text [n] and starts [n] of ONE window (token 0 opens a word whatever starts[0]
 *   says) -> probs_out, one per word, at most n; returns the number of words, or an error code (< 0).
 * ohw_state_score: for the windows of the last encode (batch = its batch), the arguments of ohw_state_align.  tokens
 *   [batch][stride], n_tokens[b] = 0 skips the window (its rows of the outputs are left alone).  scores_out [batch][stride + 1]:
 *   entry i < n_tokens[b] scores t_i, entry n_tokens[b] scores end-of-text.  The caller may score any text, not only what a decode
 *   kept: external hypotheses, an expected utterance, corrected text.
 *   start_idx_out == NULL: score only - no alignment heads are needed, no tap runs, n_frames is not read (may be NULL).
 *   start_idx_out != NULL: the alignment of ohw_state_align too, from the SAME replay (one run_decoder_step per chunk serves the
 *   tap and the score): start_idx_out and the "align_*" fetches are those of ohw_state_align on the same arguments, bit for bit.
 *   After each chunk's step token_score_kernel reads the chunk's logits, which the logits GEMM stores for all 8 rows per window.
 *   That buffer, f32 [max_batch * 8][ld] (159 MB at 96 windows and 51 866 columns), is made by the first scoring call and
 *   released by ohw_state_set_score_buffers(st, 0).  on = 1 makes it ahead of time; on = 2 also keeps, from then on, the rows
 *   of every call's LAST window for the "score_logits" fetch below (f32 [n_text_ctx / 2 + 16][ld], one device copy per chunk).
 *   It honours ohw_state_set_audio_ctx, ohw_state_set_window_ctx, the packed encoder, the language table and
 *   ohw_state_set_batch_invariant.  Refused with OHW_E_INVALID_ARG before any launch: a null argument; batch other than the last
 *   encode's; a token id < 0 or >= eot (window and position named); n_tokens[b] < 0, > stride or > n_text_ctx / 2 (window named);
 *   with start_idx_out: no head list, n_frames NULL or n_frames[b] < 0; a call under another audio context or other per-window
 *   contexts than the last encode; a language table with a pending entry (window named).
 *   Side effects: ohw_state_align's - AFTER THE CALL THE STATE'S SELF K/V IS STALE (every decode entry starts at position 0 and
 *   rewrites it), the logits rows of the windows hold the last chunk's last position, the tallies count the steps.
 * ohw_state_fetch gains "score_logits" (under ohw_state_set_score_buffers(st, 2); batch = the last ohw_state_score's): the
 *   all-rows logits [n_chunks * 8][n_vocab] of window batch - 1 of that call, n_chunks = ceil((P + max n_tokens + 1) / 8); row r =
 *   position r of the sequence, rows behind the window's own positions are those of the eot padding. */
typedef struct { float logit, lse_text, lse_all; int32_t top_id; float top_logit; } ohw_token_score;
int ohw_state_score(ohw_state* st, const ohw_sample_params* p, const int32_t* tokens, int stride, const int32_t* n_tokens,
                    int batch, ohw_token_score* scores_out /* [batch][stride + 1] */,
                    const int32_t* n_frames /* NULL unless aligning */, int32_t* start_idx_out /* NULL: score only */);
int ohw_state_set_score_buffers(ohw_state* st, int on);
int ohw_token_score_host(const float* x, int n_vocab, int eot, int target, ohw_token_score* out);
int ohw_token_prob_host(const ohw_token_score* s, float* logprob_text, float* logprob_all, float* top_logprob_text);
int ohw_word_probs_host(const float* logprob_text, const int32_t* starts, int n, float* probs_out);
/* ---- confidence in the engine.  ohw_engine_set_confidence(e, on): off (0) is the default and launches and allocates nothing;
 *      turning it off frees the score buffers of every state of the engine.  When on, every schedule, the seek loop,
 *      ohw_engine_transcribe_batch, _long_batch and _speech score the kept pass of each window on the state that decoded it, before
 *      that state's next encode (ohw_state_score) - in the SAME replay as the alignment when word timestamps are on too, alone when
 *      they are not.  Windows dropped by the no-speech rule or without a text token get none.  Tokens, text, times, quality records
 *      and candidates do not change.  Results of the last ohw_engine_transcribe, valid until the next call:
 *   token probs   one entry per kept text token (no alignment needed): its id, the index of its window, logprob_text
 *                 (logit - lse_text, openai's), logprob_all (logit - lse_all), logprob_decode = the kept pass's OWN token_logprobs
 *                 entry of that token (whisper.cpp's plog: taken behind every logit rule and the temperature; copied, not
 *                 recomputed), the unconstrained model's best text token and its logprob_text;
 *   word probs    one entry per word (ohw_word_starts_host on the window's text tokens; no alignment heads needed): the span of
 *                 the word in the text and ohw_word_probs_host's probability.  With word timestamps on, entry i covers the span
 *                 of ohw_engine_last_words entry i;
 *   segment info  one entry per ohw_engine_last_segments entry: the mean of its text tokens' logprob_text (NaN for a segment
 *                 whose window was not scored), its window's no_speech_prob and temperature.
 *   ohw_engine_batch_confidence: the same three arrays for recording i of the last batch call (any pointer may be NULL).
 *   ohw_pool_set_confidence: the setting on every engine of the pool; ohw_pool_transcribe gathers the three arrays in recording
 *   order like the times: ohw_pool_last_token_probs / _last_word_probs / _last_segment_info.                              */
typedef struct { int32_t id, window; float logprob_text, logprob_all, logprob_decode; int32_t top_id; float top_logprob_text; } ohw_token_prob;
typedef struct { size_t text_off, text_len; float probability; } ohw_word_prob;
typedef struct { float avg_logprob_text, no_speech_prob, temperature; } ohw_segment_info;
int ohw_engine_set_confidence(struct ohw_engine* e, int on);
int ohw_engine_last_token_probs(struct ohw_engine* e, const ohw_token_prob** t, int* n);
int ohw_engine_last_word_probs(struct ohw_engine* e, const ohw_word_prob** w, int* n);
int ohw_engine_last_segment_info(struct ohw_engine* e, const ohw_segment_info** s, int* n);
int ohw_engine_batch_confidence(struct ohw_engine* e, int i, const ohw_token_prob** token_probs, int* n_token_probs,
                                const ohw_word_prob** word_probs, int* n_word_probs, const ohw_segment_info** segment_info, int* n_segments);
/* ohw_engine_score_batch: scores text the CALLER supplies - external hypotheses to rescore, an expected utterance to verify,
 * corrected text - against n recordings of 16 kHz audio, each at most 30 s (one window) and at most n_text_ctx / 2 text tokens
 * (ids 0 .. eot - 1; recording i's are tokens[offsets[i] .. offsets[i + 1]), offsets [n + 1]).  The recordings go through
 * ohw_engine_transcribe_batch's front end (validation, longest first, max_batch at a time, audio_ctx "auto" if set, language
 * detection if set) and each is then scored with ohw_state_score; the confidence setting need not be on.  results [n]: the
 * ohw_token_prob list (window 0, logprob_decode NaN: nothing was decoded; the pointer is the engine's, valid until its next
 * call), the end-of-text row, and the sum of logprob_all over the tokens and end-of-text - the sequence log-likelihood.  A
 * recording with no token gets no scores (n_tokens 0, NaN).  N candidates for one recording: pass it N times (N encodes).
 * Texts: ohw_tokenize first, with the caveat of command lists - it is not BPE merging; token ids are the exact form.
 * (The entry itself is declared below, behind ohw_audio_span.)                                                            */
typedef struct { const ohw_token_prob* tokens; int32_t n_tokens; ohw_token_prob eot; float sum_logprob_all; } ohw_score_result;
int ohw_pool_set_confidence(struct ohw_pool* p, int on);
int ohw_pool_last_token_probs(struct ohw_pool* p, const ohw_token_prob** t, int* n);
int ohw_pool_last_word_probs(struct ohw_pool* p, const ohw_word_prob** w, int* n);
int ohw_pool_last_segment_info(struct ohw_pool* p, const ohw_segment_info** s, int* n);

/* per-stage device time of the last calls on this state, in milliseconds (reference logs the     */
/* same split per job: src/queue/worker.rs:170-180)                                               */
typedef struct { float mel_ms, encode_ms, decode_ms, total_ms; int32_t decode_steps; } ohw_timings;
int ohw_state_timings(ohw_state* st, ohw_timings* t);

/* per-kernel-class timing with HIP events on the state's stream (bench.py's roofline leg).        */
/* Classes = kernels: 1 encoder/cross-KV MFMA GEMM, 2 encoder attention, 3 decoder cross-attention, */
/* 4..8 the instantiations of the decoder weight-streaming GEMM (residual-accumulate out-projections */
/* and mlp.2; LN+QKV; LN+cross-query; LN+mlp.0+GELU; logits).  work = algorithmic flops (1, 2) or    */
/* bytes (3..8) summed over the launches between begin and end.                                     */
enum { OHW_PROF_NONE = 0, OHW_PROF_ENC_GEMM = 1, OHW_PROF_ENC_ATTN = 2, OHW_PROF_DEC_XATTN = 3, OHW_PROF_DEC_GEMM = 4,
       OHW_PROF_DEC_GEMM_QKV = 5, OHW_PROF_DEC_GEMM_XQ = 6, OHW_PROF_DEC_GEMM_FC1 = 7, OHW_PROF_DEC_GEMM_LOGITS = 8 };
int ohw_state_profile_begin(ohw_state* st, int kernel_class);
int ohw_state_profile_end(ohw_state* st, int64_t* launches, double* total_ms, double* work);

/* ---- WhisperEngine mirror (reference src/engine/whisper.rs:110-387): the host driver written   */
/*      in C++ because no Rust toolchain exists in the build image --------------------------------- */
typedef struct ohw_engine ohw_engine;
/* WhisperEngine::new(model_path, language, translate, use_gpu) — reference :129-179              */
int ohw_engine_new(const char* model_path, const char* language, int translate, int use_gpu, int device,
                   int dtype, int max_batch, ohw_engine** out);
/* WhisperEngine::transcribe(&AudioBuffer) — reference :204-310.  Text is copied into text_buf     */
/* (UTF-8, NUL-terminated, truncated to text_cap).  language_out: >= 8 bytes.                      */
int ohw_engine_transcribe(ohw_engine* e, const float* samples, int64_t n, uint32_t sample_rate,
                          char* text_buf, size_t text_cap, char* language_out, uint64_t* duration_ms,
                          ohw_audio_info* info);
/* full text of the last transcribe (owned by the engine until the next call): a 2 h file can exceed any   */
/* fixed text_buf; text_buf receives a truncated copy, this returns everything.                              */
int ohw_engine_last_text(ohw_engine* e, const char** text, size_t* len);
/* whisper.cpp's per-window decode policy, which the reference inherits because it sets none of these
 * (reference src/engine/whisper.rs:243-263 -> whisper_full_default_params; recalled from
 * upstream, unpinned):
 *   - exits of the decode loop: end-of-text; a timestamp that leaves less than 1 s of audio; failure when the loop
 *     reaches n_max without a timestamp past the middle of the window (the repetition guard) or when end-of-text comes
 *     with no timestamp while audio is left;
 *   - acceptance: not failed, token-frequency entropy of the last 32 tokens >= entropy_thold, and not
 *     (avg_logprob < logprob_thold while no_speech_prob < no_speech_thold); a pass that is not accepted is decoded again
 *     at temperature += temperature_inc (up to 1.0), drawn from std::mt19937(0) through std::discrete_distribution on
 *     the window's resident cross K/V: by default the host samples every step (ohw_decode_active + ohw_sample_host), with
 *     ohw_engine_set_fallback_device(e, 1) the device does (ohw_sample_pass, the host's generator pre-drawn); the last
 *     temperature is accepted whatever it gives;
 *   - no speech: a window with no_speech_prob > no_speech_thold and avg_logprob < logprob_thold yields no text.
 * temperature_inc <= 0 keeps every window at T = 0 (what bench.py times: SURVEY.md 8d). */
typedef struct { float temperature_inc, entropy_thold, logprob_thold, no_speech_thold; } ohw_decode_policy;
void ohw_default_decode_policy(ohw_decode_policy* q);   /* 0.2, 2.4, -1.0, 0.6 */
int ohw_engine_set_decode_policy(ohw_engine* e, const ohw_decode_policy* q);
/* host only: the engine's own copy of the two rules above, for tests.  ohw_seq_eval_host judges one sampled sequence
 * (tokens[0..n), end-of-text last when it was sampled, plogs its log-probabilities) of the window [seek, seek_end) in 10 ms
 * frames: where the loop would have stopped (n_sampled), result_len, seek_delta, the tokens that reach the text (n_keep: all
 * before the exit in the fixed-cut modes, result_len in OHW_WINDOW_SEEK), failed / completed, and the two scores.
 * ohw_needs_fallback_host: 1 when a pass so judged goes to the next temperature, 0 when it is kept (always at the last). */
typedef struct { int32_t n_sampled, result_len, n_keep, seek_delta, failed, completed; float avg_logprob, entropy; } ohw_seq_eval;
int ohw_seq_eval_host(const ohw_special_tokens* tok, const int32_t* tokens, const float* plogs, int n, int seek, int seek_end, int n_max,
                      int no_timestamps, int window_mode, ohw_seq_eval* out);
int ohw_needs_fallback_host(const ohw_seq_eval* ev, const ohw_decode_policy* q, float no_speech_prob, int is_last);
/* on != 0: the temperature fallback samples on the device (ohw_sample_pass, one call per rung) instead of the host; the
 * same passes, generators and decisions.  Default 0. */
int ohw_engine_set_fallback_device(ohw_engine* e, int on);
/* per window of the last transcribe, for the pass that was kept */
typedef struct {
  int32_t n_tokens;        /* tokens that reached the text / ohw_engine_last_tokens (0 for a no-speech window) */
  float avg_logprob;       /* over the first result_len tokens (whisper.cpp avg_logprobs; -inf when result_len == 0) */
  float entropy;           /* of the last 32 of them */
  int32_t would_fallback;  /* the T = 0 pass failed the acceptance test */
  float temperature;       /* of the kept pass */
  float no_speech_prob;
  int32_t no_speech;       /* dropped by the no-speech rule */
  int32_t seek_delta;      /* 10 ms frames the window covers: 3000 unless a timestamp ended it (what the seek loop advances by) */
  int32_t result_len;      /* whisper.cpp result_len: tokens up to and including the last timestamp */
  int32_t failed;          /* the kept pass ended in one of the loop's failure exits */
} ohw_window_quality;
int ohw_engine_last_quality(ohw_engine* e, const ohw_window_quality** q, int* n_windows);
/* every decode pass of the last transcribe, flat: {window index, temperature * 1000, n, n sampled tokens
 * (end-of-text included when it was sampled)} repeated - what a parity check walks pass by pass */
int ohw_engine_last_trace(ohw_engine* e, const int32_t** data, int* n);
/* How audio longer than 30 s is windowed.  FIXED (default): host-side cuts every 30 s, windows batched
 * (BASELINE.json north_star).  SEEK: whisper.cpp's sequential loop as recalled (unpinned): the
 * next window starts at the last timestamp token of the previous one (seek += 2 * (ts - ts_begin) frames of
 * 10 ms, or 3000 when no timestamp was produced), tokens after that timestamp are dropped and re-decoded;
 * stops when less than 1 s is left.  One window at a time, so batch = 1.
 * FIXED_RECORDING_MEL: the cuts, batching and schedules of FIXED, but every window is cut from the spectrogram of the WHOLE
 * recording (ohw_recording_set / ohw_mel_seek): one clamp maximum for all windows and real samples across the 30 s marks -
 * what whisper.cpp's front end gives a recording handed over in one call - instead of treating each cut as its own call. */
enum { OHW_WINDOW_FIXED = 0, OHW_WINDOW_SEEK = 1, OHW_WINDOW_FIXED_RECORDING_MEL = 2 };
int ohw_engine_set_window_mode(ohw_engine* e, int mode);
/* measurement knob (bench.py --pool; SURVEY.md 8d "decode length is pinned"): n_tokens > 0 makes every window decode exactly
 * that many tokens with end-of-text suppressed (ohw_sample_params.force_len; use with temperature_inc = 0: a forced sequence
 * fails whisper.cpp's acceptance test by construction); 0 (default) = the reference's behaviour.                         */
int ohw_engine_set_force_len(ohw_engine* e, int n_tokens);
/* beam search as the T = 0 strategy of every transcribe of the engine (whisper.cpp's WHISPER_SAMPLING_BEAM_SEARCH): k = 0
 * (default) = greedy, k = 2..5 = ohw_beam_search_ex with k beams per window.  OHW_E_INVALID_ARG for another k, for
 * k > max_batch, and together with ohw_engine_set_force_len (whichever setter comes second fails).  Everything else of a
 * transcribe stays: window modes and the seek loop, ohw_engine_transcribe_batch(_lang) and _long_batch, the acceptance test,
 * the no-speech rule, the temperature ladder, segments, word timestamps, prompts, languages and audio contexts per window.
 *   - a decode batch holds floor(max_batch / k) windows (k decoder rows per window); batch cutting takes that number
 *   - the search's winner - with end-of-text when it came from the finished pool - is judged by whisper.cpp's bookkeeping and
 *     cut at the first of its loop exits, like a sampled pass; it is traced at temperature 0 (ohw_engine_last_trace).
 *     DEVIATION: whisper.cpp applies its loop exits to every decoder during the search; beam search is not causal, so here they
 *     are applied to the winner after it
 *   - passes at T > 0 are the unchanged ladder (whisper.cpp as recalled: at t_cur > 0 the beam strategy samples, best_of:
 *     ohw_engine_set_best_of gives those passes their candidates)
 *   - the LANES / PIPELINE schedules are not used: a call with beam on runs one batch after the other on the engine's own state */
int ohw_engine_set_beam_size(ohw_engine* e, int k);
/* best-of sampling above T = 0 (whisper.cpp's best_of, for the greedy and the beam strategy alike; restated from memory,
 * unpinned - DESIGN.md section 9 marks the definitions): n = 1 (default) = today's ladder, n = 2..5 = every rung with T > 0
 * samples n candidates per pending window and keeps one.  OHW_E_INVALID_ARG outside 1..5, for n > max_batch, and together with
 * ohw_engine_set_force_len (whichever setter comes second fails).  Nothing changes at T = 0 or when temperature_inc <= 0.
 *   - candidate j draws from its own std::mt19937(j) (ohw_rng_new(j)), which lives where today's one generator lives (per cut;
 *     per recording and call in the seek loops); candidate 0 is today's decoder.  After a rung candidate j's generator has
 *     advanced by the draws its own cut pass consumed
 *   - every candidate is cut at the loop exits and judged like today's one row; ohw_best_of_pick_host picks: a candidate is
 *     out when it failed or its entropy is below entropy_thold; of the rest the highest avg_logprob wins, the lowest j among
 *     equals; all out: candidate 0.  The kept candidate is the rung's pass from there on (acceptance test, no-speech rule,
 *     carry, segments, alignment); ohw_engine_last_trace records it, ohw_engine_last_candidates all of them
 *   - with n > 1 the rungs are sampled on the device (ohw_sample_pass_n) whatever ohw_engine_set_fallback_device says
 *   - a decode batch holds floor(max_batch / max(n, beam size, 1)) windows; calls with n > 1 run one batch after the other on
 *     the engine's own state, like beam calls                                                                             */
int ohw_engine_set_best_of(ohw_engine* e, int n);
/* windows per decode batch of an engine with these settings: floor(max_batch / max(best_of, beam_size, 1)), what every
 * transcribe path cuts its batches by (host only); OHW_E_INVALID_ARG (negative) for max_batch < 1, a beam size other than 0 or
 * 2..5, best_of outside 1..5, or a result of 0 */
int ohw_batch_windows_host(int max_batch, int beam_size, int best_of);
/* the pick of one rung over n judged candidates (host only; the engine calls this function): *kept = the candidate's index */
int ohw_best_of_pick_host(const ohw_seq_eval* ev, int n, const ohw_decode_policy* q, int* kept);
/* every best-of rung of the last transcribe, flat: {window index, temperature * 1000, N, kept j}, then per candidate {n, n
 * tokens (cut; end-of-text included when it was sampled)}; rungs in the order of ohw_engine_last_trace.  Empty when best_of = 1 */
int ohw_engine_last_candidates(ohw_engine* e, const int32_t** data, int* n);
/* the log-probabilities of those candidates' tokens, in the record's order and nothing else: what ohw_seq_eval_host needs to
 * judge a recorded candidate again */
int ohw_engine_last_candidate_logprobs(ohw_engine* e, const float** data, int* n);
/* reduced audio context of every window ohw_engine_transcribe runs (ohw_state_set_audio_ctx on the engine's own, pipeline
 * and lane states): 0 (default) = off, the full context; n > 0 = that context for every window of every window mode and
 * schedule - a transcribe in which some window holds samples past n * 320 fails with OHW_E_INVALID_ARG naming the window
 * (audio is never dropped silently); -1 = auto: a recording that fits one window runs at ohw_audio_ctx_for(n_samples),
 * anything longer at the full context.                                                                                   */
int ohw_engine_set_audio_ctx(ohw_engine* e, int n);
/* an initial prompt (whisper.cpp's initial_prompt / prompt_tokens: names, jargon, spelling hints): text (tokenized with
 * ohw_tokenize; NULL or "" clears) or token ids (n = 0 clears; ids outside the vocabulary: OHW_E_INVALID_ARG).  A prompt longer
 * than n_text_ctx / 2 - 1 tokens keeps its last n_text_ctx / 2 - 1.  Every window of every schedule (fixed cuts, the seek loop,
 * ohw_engine_transcribe_batch, lanes, the pool) decodes behind it through ohw_state_set_window_prompt; it is not part of the
 * result.  Temperature ladder: passes with T < 0.5 decode behind the prompt, the table is cleared before the first pass with
 * T >= 0.5 and set again for the next batch.  Off by default: with no prompt ever set nothing takes a new path.             */
int ohw_engine_set_initial_prompt(ohw_engine* e, const char* text);
int ohw_engine_set_initial_prompt_tokens(ohw_engine* e, const int32_t* tokens, int n);
/* hot phrases on every state the engine decodes on (ohw_state_set_phrase_table states the rule and both forms) */
int ohw_engine_set_hot_phrases(ohw_engine* e, const char* const* texts, const float* boosts, int n);
int ohw_engine_set_hot_phrases_tokens(ohw_engine* e, const int32_t* tokens, const int32_t* offsets, const float* boosts, int n_phrases);
/* repetition penalty and no-repeat n-gram size on every state the engine decodes on (ohw_state_set_repeat_rule states the rule);
 * (1.0, 0), the default, is off */
int ohw_engine_set_repetition(ohw_engine* e, float penalty, int ngram);
/* a command list on every state the engine decodes on (ohw_state_set_command_table states the rule, both forms and the hits);
 * ohw_engine_batch_commands: the hits of recording i of the last ohw_engine_transcribe_batch / _long_batch / _speech call */
int ohw_engine_set_commands(ohw_engine* e, const char* const* texts, int n, float penalty);
int ohw_engine_set_commands_tokens(ohw_engine* e, const int32_t* tokens, const int32_t* offsets, int n_phrases, float penalty);
int ohw_engine_last_commands(ohw_engine* e, const ohw_command_hit** hits, int* n);
int ohw_engine_batch_commands(ohw_engine* e, int i, const ohw_command_hit** hits, int* n);
/* carried context in the seek loops (whisper.cpp's prompt_past / n_max_text_ctx, as recalled): max_tokens 0 (default) = off,
 * -1 = on with the full cap of ohw_prompt_clip_host, n > 0 = on with at most n tokens (whisper.cpp's --max-context); below -1:
 * OHW_E_INVALID_ARG.  It applies to OHW_WINDOW_SEEK in ohw_engine_transcribe and to ohw_engine_transcribe_long_batch, one
 * history per recording and call (in the long batch it follows the recording, not the slot).  The history starts as the initial
 * prompt (which is then only its seed and scrolls away; it is not put in front of every window in addition); a window's T = 0
 * pass and the ladder's passes below T = 0.5 decode behind the history's tail, the table is cleared before the first pass with
 * T >= 0.5; after the window ohw_carry_step_host moves the history on.  In OHW_WINDOW_FIXED, OHW_WINDOW_FIXED_RECORDING_MEL and
 * ohw_engine_transcribe_batch every cut or recording is its own whisper_full call: the setting has no effect there.
 * ohw_pool_set_carry_context: the setting on every engine of the pool.
 * ohw_engine_last_context: the context tokens ([prev] not included; n = 0: none) window `window` of the last
 * ohw_engine_transcribe was decoded behind at T = 0 - with carry off, the initial prompt; a window out of range:
 * OHW_E_INVALID_ARG.  ohw_engine_long_batch_context: the same for window `window` of recording `rec` of the last long batch.
 * ohw_carry_step_host (host only, the function the engine itself calls): history [n_text_ctx / 2] holds *n_history tokens, oldest
 * first.  First the window's kept pass is applied: kept_temperature >= 0.5 clears the history (that pass ran without [prev]),
 * then kept[0 .. n_kept) - what the window contributed to the tokens of the result, timestamp tokens included - is appended and
 * the history keeps its last n_text_ctx / 2 tokens.  Then the next window's context is written to context_out
 * [n_text_ctx / 2 - 1]: with max_tokens = 0 nothing, else the tail ohw_prompt_clip_host keeps, cut to its last max_tokens when
 * max_tokens > 0.  n_kept = 0 at temperature 0 only derives the context (the first window of a call).                      */
int ohw_engine_set_prefill_chunk(ohw_engine* e, int positions);     /* ohw_state_set_prefill_chunk on every state of the engine */
int ohw_engine_set_carry_context(ohw_engine* e, int max_tokens);
int ohw_engine_last_context(ohw_engine* e, int window, const int32_t** tokens, int* n);
int ohw_engine_long_batch_context(ohw_engine* e, int rec, int window, const int32_t** tokens, int* n);
int ohw_carry_step_host(int32_t* history, int* n_history, int n_text_ctx, const int32_t* kept, int n_kept, float kept_temperature,
                        int max_tokens, int32_t* context_out, int* n_context_out);
/* Stitched windows: the fixed cuts overlap and neighbouring windows' tokens are merged where they agree (DESIGN.md sections 6
 * and 9).  ohw_engine_set_stitch(e, overlap_ms): 0 (default) = off, every path gives the bits it gave before; else a multiple
 * of 20 in [1000, 15000] (anything else: OHW_E_INVALID_ARG).  It applies to ohw_engine_transcribe in OHW_WINDOW_FIXED and
 * OHW_WINDOW_FIXED_RECORDING_MEL, all three schedules; it has NO effect on OHW_WINDOW_SEEK, ohw_engine_transcribe_batch,
 * _long_batch, _speech or on an engine of a pool that takes a share of a recording.
 *   The plan (ohw_stitch_plan_host): the hop is H = 480000 - overlap_ms * 16 samples; a recording of n <= 480000 samples is one
 * window (none for n = 0), otherwise W = ceil((n - 480000) / H) + 1; window k covers samples [k * H, min(n, k * H + 480000)), so
 * the last window always reaches past the end of the one before it.  Off: H = 480000 and W = ceil(n / 480000).
 *   The seam rule (ohw_stitch_seams_host; ohw_stitch_seams is its device twin on host arrays): a seam joins window w (left) and
 * w + 1 (right); its inputs are the two windows' kept TEXT tokens (ids below end-of-text), L and R of them.  For every shift
 * i = 1 .. L + R - 1: ls = max(0, L - i), le = min(L, L + R - i), rs = max(0, i - L), re = min(R, i), m = the number of j with
 * left[ls + j] == right[rs + j], score = (double)m / (double)i + (double)i / 10000.0.  The seam takes the first i in ascending
 * order with m > 1 and a score strictly above the best so far (from 0.0): left_cut = (ls + le) / 2, right_cut = (rs + re) / 2.
 * With no such shift the seam is unmatched: shift = matches = 0, left_cut = L, right_cut = 0 - both windows stay whole.  For two
 * windows this is transformers' _find_longest_common_sequence; seams are independent of each other (a definition).
 * text_tokens [n_windows][stride], n_text [n_windows] (0 .. stride, stride <= 4096); seams_out [n_windows - 1]; n_windows <= 1
 * does nothing.  ohw_dbg_stitch: the device twin with n_guard more seams behind the output, which it fills with `sentinel` words
 * before the launch (seams_out [n_windows - 1 + n_guard]).
 *   The ranges (ohw_stitch_ranges_host): window w keeps text tokens [rc, max(rc, lc)) - rc the right_cut of the seam on its left
 * (0 for the first window), lc the left_cut of the seam on its right (its text count for the last).  In a window's kept tokens
 * the range runs from the position of text token rc (index 0 when rc = 0) to the position of text token lc (all kept tokens
 * when lc is the text count): timestamp tokens of an uncut end stay, and so do those in between.
 *   Segments are formed by ohw_segments_host on the window's whole kept tokens and clipped to the range
 * (ohw_stitch_clip_segment_host: returns 0 for a segment wholly outside [first, end), else 1 with *out the retained part; an end
 * the range cut takes the seam time of that side, clamped into the segment's own [t0, t1]).  The seam time is the middle of the
 * shared audio on the recording's clock: (start of the right window + end of the left window) / 2.
 *   ohw_engine_last_seams: the seams of the last stitched ohw_engine_transcribe (none with stitch off or one window).
 * ohw_engine_last_window_tokens: every window's kept tokens before the cut, window w at tokens[offsets[w] .. offsets[w + 1]);
 * n_windows = 0 when the last transcribe was not stitched.  token_times / token_probs list the retained text tokens only; words
 * and word probabilities are formed over a window's retained tokens; quality records, contexts, command hits and the trace stay
 * one per window.                                                                                                            */
typedef struct { int32_t left_window, shift, matches, left_cut, right_cut, n_left, n_right, reserved; } ohw_seam;
int ohw_stitch_plan_host(int64_t n_samples, int overlap_ms, int64_t* hop_samples, int64_t* n_windows);
int ohw_stitch_seams_host(const int32_t* text_tokens, int stride, const int32_t* n_text, int n_windows, ohw_seam* seams_out);
int ohw_stitch_ranges_host(const ohw_seam* seams, const int32_t* n_text, int n_windows, int32_t* first_out, int32_t* end_out);
int ohw_stitch_clip_segment_host(const ohw_token_span* seg, int first, int end, float t_seam_left, float t_seam_right, ohw_token_span* out);
int ohw_stitch_seams(int device, const int32_t* text_tokens_host, int stride, const int32_t* n_text, int n_windows, ohw_seam* seams_out);
int ohw_dbg_stitch(int device, const int32_t* text_tokens_host, int stride, const int32_t* n_text, int n_windows, int n_guard, int32_t sentinel,
                   ohw_seam* seams_out);
int ohw_engine_set_stitch(ohw_engine* e, int overlap_ms);
int ohw_engine_stitch(ohw_engine* e);      /* the setting, ms */
int ohw_engine_last_seams(ohw_engine* e, const ohw_seam** seams, int* n);
int ohw_engine_last_window_tokens(ohw_engine* e, const int32_t** tokens, const int32_t** offsets, int* n_windows);
/* ohw_state_set_packed_encoder on the engine's own, pipeline and lane states, those made later included (default: what
 * OHW_ENC_PACKED gave the engine's own state).  It matters for ohw_engine_transcribe_batch under the auto context (-1): a
 * batch of mixed lengths then encodes the sum of its contexts; tokens, text and quality records do not change.             */
int ohw_engine_set_packed_encoder(ohw_engine* e, int on);
/* Several independent recordings in one call: each is its own whisper_full call of at most one 30 s window (cut as
 * OHW_WINDOW_FIXED cuts; another window mode returns OHW_E_INVALID_ARG), with its own std::mt19937(0) and its own frame count
 * as the end of the audio, decoded by the per-window policy of ohw_engine_transcribe.  Every recording passes
 * ohw_validate_audio before any device work (a failure: OHW_E_VALIDATION, ohw_last_error() names the recording's index); one
 * longer than 30 s returns OHW_E_INVALID_ARG naming its index.  The recordings are sorted by length, longest first, cut into
 * batches of max_batch and run one batch after the other on the engine's own state (no lanes, no pipeline).  The context of
 * recording i follows ohw_engine_set_audio_ctx: 0 = the full context; n > 0 = n for all (a recording with samples past n * 320
 * is refused by index); -1 = ohw_audio_ctx_for(n_i) per recording through ohw_state_set_window_ctx, the batch's envelope
 * being the largest of them.  ohw_state_set_batch_invariant is on for the whole call, so a recording's result does not depend
 * on which other recordings it was submitted with.  Results are read back per recording, in submission order, and stay
 * valid until the next ohw_engine_transcribe_batch; ohw_engine_last_* are empty after this call.                        */
typedef struct { const float* samples; int64_t n; } ohw_audio_span;
int ohw_engine_transcribe_batch(ohw_engine* e, const ohw_audio_span* recs, int n_recs, uint32_t sample_rate);
int ohw_engine_score_batch(ohw_engine* e, const ohw_audio_span* recs, int n_recs, const int32_t* tokens, const int32_t* offsets,
                           ohw_score_result* results);     /* "confidence in the engine" above */
/* result of recording i of the last ohw_engine_transcribe_batch; every out pointer may be NULL; language_out: >= 8 bytes */
/* language detection in the engine (default 0: language "auto" stays "en", as in the reference).  It applies only when the
 * engine's language is "auto"; an explicit language is unaffected, and an English-only model stays "en" without a detection.
 * ohw_engine_transcribe then detects once per call, as whisper.cpp's whisper_full does: before the schedule starts the engine's
 * own state runs the front end of window 0 alone, under the context window 0 is decoded in (the recording-wide spectrogram in
 * the recording-mel and seek modes), and ohw_state_detect_window_lang; every window of every schedule runs at that id, so the
 * tokens are those of an engine created with its code.  language_out reports the code; ohw_engine_last_language the id and
 * the detection's probability of it (prob 1 when nothing was detected).  ohw_engine_transcribe_batch detects every recording
 * on its own (all table entries OHW_LANG_DETECT after each batch's encode; greedy pass and ladder decode from the table, the
 * host-sampled ladder from one read-back per batch); ohw_engine_batch_result's language_out is then each recording's code.
 * ohw_engine_transcribe_batch_lang: the same call with lang_ids[i] = a language id or OHW_LANG_DETECT per recording, whatever
 * the engine's language and setting (ignored on an English-only model); NULL = ohw_engine_transcribe_batch.
 * ohw_pool_set_detect_language: the setting on every engine; the pool detects once, on its first engine, and hands the id on. */
int ohw_engine_set_detect_language(ohw_engine* e, int on);
int ohw_engine_last_language(ohw_engine* e, int32_t* id, float* prob);
int ohw_engine_transcribe_batch_lang(ohw_engine* e, const ohw_audio_span* recs, const int32_t* lang_ids, int n_recs, uint32_t sample_rate);
int ohw_engine_batch_result(ohw_engine* e, int i, const char** text, size_t* text_len, const int32_t** tokens, int* n_tokens,
                            const ohw_window_quality** quality, char* language_out);
/* host only: the bookkeeping of many seek loops (OHW_WINDOW_SEEK) run side by side, one window of every live recording per
 * round.  ohw_engine_transcribe_long_batch runs on this object; it can be driven without a GPU.  The rule is deterministic:
 *   - recording i ends at seek_end = 1 + (n_samples[i] - 200) / 160 frames of 10 ms and starts at seek 0;
 *   - it is live while seek_end >= 100 && seek + 100 < seek_end (a recording under 1 s is never live and takes no slot);
 *   - the live recordings wait longest first, equal lengths in submission order; there are max_batch slots, all free at first;
 *   - ohw_seek_sched_round first gives every free slot, lowest slot first, to the next waiting recording, then lists the taken
 *     slots in slot order: rec_out[b] the recording, slot_out[b] its slot, seek_out[b] its seek, fresh_out[b] = 1 when the
 *     recording has taken the slot since the last round (its samples must be uploaded).  It returns the number of entries B
 *     (the four arrays hold max_batch entries), 0 when every recording has ended, -1 on a null argument;
 *   - ohw_seek_sched_advance(s, b, seek_delta), once per entry b of the last round, moves that recording on by
 *     seek_delta > 0 ? seek_delta : 3000; a recording that is no longer live frees its slot, which the next waiting recording
 *     takes in the following round.                                                                                        */
typedef struct ohw_seek_sched ohw_seek_sched;
int ohw_seek_sched_new(const int64_t* n_samples, int n_recs, int max_batch, ohw_seek_sched** out);
int ohw_seek_sched_round(ohw_seek_sched* s, int32_t* rec_out, int32_t* slot_out, int32_t* seek_out, int32_t* fresh_out);
int ohw_seek_sched_advance(ohw_seek_sched* s, int b, int seek_delta);
void ohw_seek_sched_free(ohw_seek_sched* s);
/* Long-form batch: several independent recordings of ANY length (up to a recording slot's two hours), each through the seek
 * loop of OHW_WINDOW_SEEK, one window of every live recording in the same encode and decode batch.  The call always runs the seek
 * loop, whatever ohw_engine_set_window_mode says, on the engine's own state with ohw_state_set_batch_invariant on for the call
 * (no lanes, no pipeline, no pool).  Every recording passes ohw_validate_audio before any device work (OHW_E_VALIDATION,
 * ohw_last_error() names the index).  Per round (ohw_seek_sched_*): the fresh recordings go into their slots
 * (ohw_recording_set_slot), ohw_mel_seek_slots, ohw_encode, the greedy pass and the temperature ladder with every slot's seek,
 * end and generator, the alignment when word timestamps are on, then each window's records with its offset seek * 0.01 s.  Each
 * recording is one whisper_full call in whisper.cpp terms: its own std::mt19937(0) across all its windows, its own frame count
 * as the end of the audio, the full audio context (ohw_engine_set_audio_ctx does not apply), the initial prompt in front of every
 * window - or, under ohw_engine_set_carry_context, the recording's own carried history, which follows the recording and not its
 * slot.  Language: lang_ids as in ohw_engine_transcribe_batch_lang (NULL: the engine's language, or - with
 * ohw_engine_set_detect_language - one detection per recording, on its first window, read back once and kept for its later ones).
 * CONTRACT: recording i's text, tokens, per-window quality records (seek_delta and temperature included), segments, token and
 * word times and language are exactly those of ohw_engine_transcribe on it alone in OHW_WINDOW_SEEK at the full audio context
 * with ohw_state_set_batch_invariant on, whatever it was submitted with and in whatever order.
 * Results: ohw_engine_batch_result / ohw_engine_batch_times per recording in submission order (quality there points at the
 * recording's first window record); ohw_engine_long_batch_quality gives all of them, one per window (q NULL-able data of
 * n_windows records; 0 windows for a recording under 1 s).  ohw_engine_last_* are empty after this call.                 */
int ohw_engine_transcribe_long_batch(ohw_engine* e, const ohw_audio_span* recs, const int32_t* lang_ids, int n_recs, uint32_t sample_rate);
int ohw_engine_long_batch_quality(ohw_engine* e, int i, const ohw_window_quality** q, int* n_windows);
/* Speech-aware windows: recordings of ANY length that validation accepts; the speech is found, cut at its pauses into chunks of
 * at most 30 s and the chunks of all recordings run as ONE ohw_engine_transcribe_batch: longest first, contexts per
 * ohw_engine_set_audio_ctx, the packed encoder when set, batch-invariant kernels, on the engine's own state (no pool, lanes or
 * pipeline).  It needs OHW_WINDOW_FIXED, as ohw_engine_transcribe_batch does.  Every recording passes ohw_validate_audio before
 * any device work (OHW_E_VALIDATION, ohw_last_error() names the index).  Per recording: ohw_state_vad_frames - or the caller's
 * probabilities: probs NULL = the device detector for all; else probs[i] = {p, n, frame_samples} with p NULL / n 0 = the device
 * detector for recording i - then ohw_speech_segments_host and ohw_speech_chunks_host under ohw_engine_set_vad's settings.
 * lang_ids: as ohw_engine_transcribe_batch_lang, per recording (every chunk of a recording gets its entry; OHW_LANG_DETECT
 * detects per chunk); NULL: the engine's language or, with ohw_engine_set_detect_language, a detection per chunk.
 * CONTRACT: chunk c's tokens, log-probabilities, quality record, segments, token times and word times are exactly those of
 * ohw_engine_transcribe_batch given samples[start .. end) as a recording, the times shifted by the offset start / 16000.0 (they
 * go through the same code with that offset).  A recording's text is its chunks' untrimmed texts joined and then trimmed, the
 * way the fixed-cut path joins its windows.  A recording with no speech gives empty text, zero chunks and OHW_OK, and with no
 * chunk at all no encode or decode is launched.  Beam size, best-of, hot phrases, repetition rules, the initial prompt, word
 * timestamps and per-recording languages work as in ohw_engine_transcribe_batch.  ohw_engine_set_carry_context has NO effect:
 * chunks decode in parallel, so none can be decoded behind another's text.
 * Results: ohw_engine_batch_result / ohw_engine_batch_times per recording in submission order (token times' window = the chunk's
 * index in the recording); ohw_engine_long_batch_quality lists one record per chunk; ohw_engine_speech_chunks the chunks, their
 * count and the same quality records (any out pointer may be NULL); ohw_engine_speech_segments the segments the chunks index.
 * ohw_engine_set_vad: NULL = the defaults of ohw_default_vad_config / _vad_detector / _chunk_plan; cfg's enabled is ignored.      */
typedef struct { const float* p; int64_t n; int32_t frame_samples; } ohw_frame_probs;
int ohw_engine_set_vad(ohw_engine* e, const ohw_vad_config* cfg, const ohw_vad_detector* det, const ohw_chunk_plan* plan);
int ohw_engine_transcribe_speech(ohw_engine* e, const ohw_audio_span* recs, const ohw_frame_probs* probs, int n_recs, uint32_t sample_rate);
int ohw_engine_transcribe_speech_lang(ohw_engine* e, const ohw_audio_span* recs, const ohw_frame_probs* probs, const int32_t* lang_ids,
                                      int n_recs, uint32_t sample_rate);
int ohw_engine_speech_chunks(ohw_engine* e, int i, const ohw_speech_chunk** chunks, int* n, const ohw_window_quality** quality);
int ohw_engine_speech_segments(ohw_engine* e, int i, const ohw_speech_segment** segments, int* n);
/* host only: how ohw_engine_transcribe_batch batches n_recs recordings of n_samples[i] samples.  order_out [n_recs]: the
 * recordings' indices, longest first (equal lengths keep submission order); batch j holds order_out[j * max_batch ..];
 * ctx_out [n_recs]: the context of recording i under audio_ctx_setting (0 -> 1500, n -> n, -1 -> ohw_audio_ctx_for);
 * envelope_out [ceil(n_recs / max_batch)]: the largest context of each batch.  OHW_E_INVALID_ARG naming the index for a
 * recording of more than 480000 samples or one a fixed n does not cover (the first such in submission order).              */
int ohw_batch_plan(const int64_t* n_samples, int n_recs, int max_batch, int audio_ctx_setting, int32_t* order_out, int32_t* ctx_out,
                   int32_t* envelope_out);
/* How audio of more than max_batch windows is overlapped on the device (the reference transcribes one buffer at a time,
 * src/queue/worker.rs:100-160; results are identical under every schedule):
 *   SEQUENTIAL  one batch after the other;
 *   PIPELINE    front end (mel, encoder, cross K/V) of batch i+1 on OHW_ENGINE_ENC_CUS compute units beside the decode of
 *               batch i on the rest (round 1's schedule);
 *   LANES       (default) groups of up to `lanes` lanes, each of up to `merge` batches of max_batch windows (dealt evenly):
 *               a lane takes its windows through ONE front-end pass and decodes them as ONE batch; the lanes' front ends run
 *               one after the other on every compute unit, then their decodes side by side, each on its own CU-masked
 *               stream and host thread - a decode alternates an HBM-bound kernel with a latency-bound chain, several of
 *               them together keep HBM busy, and a larger decode batch streams the decoder's weights once for all its rows.
 * The schedule's extra states and streams are made when a long input first needs them (a lane's state holds up to
 * merge x max_batch windows: 245.76 MB of cross K/V per window at large-v3); environment defaults:
 * OHW_ENGINE_SCHEDULE = sequential | pipeline | lanes, OHW_ENGINE_LANES (4), OHW_ENGINE_MERGE (3), OHW_ENGINE_ENC_CUS (96). */
enum { OHW_SCHEDULE_SEQUENTIAL = 0, OHW_SCHEDULE_PIPELINE = 1, OHW_SCHEDULE_LANES = 2 };
int ohw_engine_set_schedule(ohw_engine* e, int schedule, int lanes /* 0 = keep */, int merge /* 0 = keep */);
/* tokens of the last transcribe, per 30 s window concatenated (for parity tests)                  */
int ohw_engine_last_tokens(ohw_engine* e, const int32_t** tokens, int* n);
/* WhisperEngine::benchmark(safety_margin) — reference :334-387                                    */
int ohw_engine_benchmark(ohw_engine* e, float safety_margin, float* overhead_secs, float* recommended_chunk_interval,
                         float* test_audio_secs);
void ohw_engine_free(ohw_engine* e);
ohw_state* ohw_engine_state(ohw_engine* e);
ohw_ctx* ohw_engine_ctx(ohw_engine* e);
/* ---- multi-GPU pool behind the boundary.  The reference has no multi-GPU code, only the intent:
 *      requirement F14 "distribute transcriptions across multiple GPUs on a single machine" (reference REQUIREMENTS.md:26)
 *      and the config keys `[gpu] auto_detect / devices` that today do nothing (src/config.rs:921-929).  One engine and
 *      one host thread per listed device.  The model file is read ONCE (device_ids[0]); its resident weight arena reaches
 *      the other devices in one broadcast over xGMI: RCCL (ncclCommInitAll + ncclBroadcast, loaded with dlopen at run
 *      time) or peer-to-peer copies when RCCL cannot be loaded, OHW_POOL_BCAST=peer is set, or a device is listed twice.
 *      ohw_pool_transcribe has ohw_engine_transcribe's contract; the fixed 30 s windows of the recording are dealt
 *      round-robin (window w -> device w mod n) with no collective in the data path, results gathered on the host in
 *      recording order (the seek-loop window mode is sequential and runs on device_ids[0] alone). ----------------- */
typedef struct ohw_pool ohw_pool;
int ohw_pool_create(const char* model_path, const char* language, int translate, const int* device_ids, int n_devices,
                    int dtype, int max_batch, ohw_pool** out);
/* the same pool around procedural weights made on device_ids[0] (ohw_ctx_create_synthetic) instead of a file read: what
 * bench.py --pool and the tests use where no model file exists */
int ohw_pool_create_synthetic(const ohw_hparams* hp, uint32_t seed, const char* language, int translate, const int* device_ids,
                              int n_devices, int dtype, int max_batch, ohw_pool** out);
int ohw_pool_set_force_len(ohw_pool* p, int n_tokens);                     /* ohw_engine_set_force_len on every engine */
int ohw_pool_set_beam_size(ohw_pool* p, int k);                              /* ohw_engine_set_beam_size on every engine */
int ohw_pool_set_schedule(ohw_pool* p, int schedule, int lanes, int merge); /* ohw_engine_set_schedule on every engine */
int ohw_pool_transcribe(ohw_pool* p, const float* samples, int64_t n, uint32_t sample_rate, char* text_buf, size_t text_cap,
                        char* language_out, uint64_t* duration_ms, ohw_audio_info* info);
int ohw_pool_last_text(ohw_pool* p, const char** text, size_t* len);
int ohw_pool_last_tokens(ohw_pool* p, const int32_t** tokens, int* n);
int ohw_pool_last_quality(ohw_pool* p, const ohw_window_quality** q, int* n_windows);
int ohw_pool_set_decode_policy(ohw_pool* p, const ohw_decode_policy* q);
int ohw_pool_set_fallback_device(ohw_pool* p, int on);                    /* ohw_engine_set_fallback_device on every engine */
/* the window mode of EVERY engine of the pool (ohw_engine_set_window_mode): ohw_pool_transcribe rejects a pool whose engines
 * disagree.  All three modes give the single engine's tokens: each device is handed the whole recording and cuts its own
 * windows w, w + n, ... from it (in FIXED_RECORDING_MEL from the recording-wide spectrogram).                              */
int ohw_pool_set_window_mode(ohw_pool* p, int mode);
int ohw_pool_set_initial_prompt(ohw_pool* p, const char* text);           /* ohw_engine_set_initial_prompt on every engine */
int ohw_pool_set_hot_phrases(ohw_pool* p, const char* const* texts, const float* boosts, int n);   /* ohw_engine_set_hot_phrases on every engine */
int ohw_pool_set_repetition(ohw_pool* p, float penalty, int ngram);       /* ohw_engine_set_repetition on every engine */
int ohw_pool_set_commands(ohw_pool* p, const char* const* texts, int n, float penalty);   /* ohw_engine_set_commands on every engine */
int ohw_pool_set_best_of(ohw_pool* p, int n);                             /* ohw_engine_set_best_of on every engine */
int ohw_pool_set_carry_context(ohw_pool* p, int max_tokens);              /* ohw_engine_set_carry_context on every engine */
int ohw_pool_set_audio_ctx(ohw_pool* p, int n);                           /* ohw_engine_set_audio_ctx on every engine */
int ohw_pool_set_packed_encoder(ohw_pool* p, int on);
int ohw_pool_set_detect_language(ohw_pool* p, int on);                     /* ohw_engine_set_detect_language on every engine */                     /* ohw_engine_set_packed_encoder on every engine */
/* "" or why the RCCL broadcast was given up for peer copies.  After either kind every replica's weight buffers are compared
 * with device_ids[0]'s (64-bit digests); a mismatch fails ohw_pool_create with OHW_E_LOAD_FAILED naming the device.          */
const char* ohw_pool_broadcast_note(const ohw_pool* p);
int ohw_pool_n_devices(const ohw_pool* p);
const char* ohw_pool_broadcast_kind(const ohw_pool* p);   /* "none" (one device), "rccl" or "peer" */
ohw_engine* ohw_pool_engine(ohw_pool* p, int i);           /* the i-th device's engine (borrowed) */
void ohw_pool_free(ohw_pool* p);

/* lang id -> ISO code ("unknown" outside 0..98): reference lang_id_to_code :627-731               */
const char* ohw_lang_id_to_code(int32_t id);
/* ISO code -> lang id, -1 if unknown */
int32_t ohw_lang_code_to_id(const char* code);

/* ---- diagnostics (tests) ----------------------------------------------------------------------- */
const char* ohw_last_error(void);
int ohw_abi_version(void);
/* copy an internal activation to the host as f32: what = "mel" [B][n_mels][3000], "conv1"        */
/* [B][3000][d], "stem" / "block0" / "enc" [B][1500][d], "xk<l>" / "xv<l>" [B][1500][d]            */
/* (under a reduced audio context C, "stem" / "block0" / "enc" / "xk<l>" / "xv<l>" are [B][C][d]),   */
/* "mel_t" [B][3002][128]: the 16-bit time-major image conv1 reads, pad rows and channels included; */
/* "sample_slots" [batch][n_text_ctx]: the kv_slot table of the last ohw_sample_pass_n, batch = its   */
/* n_windows * best_of rows (entries are cache row indices, exact in f32)                            */
/* "logits" [batch][n_vocab]: the first batch decoder rows (at most max_batch) of the last decoder   */
/* step's logits as its sampler saw them: the hot-phrase boost included while a table is set         */
/* and the repetition rule's changes while it is on (ohw_state_set_repeat_rule)                      */
/* and the command list's while one is set (ohw_state_set_command_table)                            */
int ohw_state_fetch(ohw_state* st, const char* what, int batch, float* out, int64_t out_elems);
/* 64-bit digest of the index-th resident weight buffer (engine layout); returns OHW_E_INVALID_ARG  */
/* past the last buffer.  Lets tests prove "synthetic ctx == ctx loaded from the synthetic file".  */
int ohw_ctx_weight_digest(const ohw_ctx* ctx, int index, char* name_out /* >= 64 bytes */, uint64_t* digest);
/* ggml block dequantisation: `blocks` holds n / 32 blocks of ttype 2 (Q4_0, 18 B), 3 (Q4_1, 20 B), 6 (Q5_0, 22 B),       */
/* 7 (Q5_1, 24 B) or 8 (Q8_0, 34 B) as stored in a model file, out receives n floats; n % 32 == 0.  The host twin needs no  */
/* device and defines the result bit for bit (fp32 after widening d / m, multiply then add, no fused multiply-add); the   */
/* dbg entry copies the blocks to `device`, runs the loader's kernel on them and copies the result back.                   */
int ohw_dequantize_host(int ttype, const void* blocks, int64_t n, float* out);
int ohw_dbg_dequantize(int device, int ttype, const void* blocks_host, int64_t n, float* out_host);
/* kernel-level entry points on raw device pointers (tests against a torch fp32 reference)         */
int ohw_dbg_gemm(int dtype, const void* A, const void* W, const float* bias, void* out, int64_t M, int64_t N,
                 int64_t K, int epilogue, void* stream);
/* the short-window encoder GEMM (gemm_small.hip: 64x64 tiles, four times the workgroups of ohw_dbg_gemm's kernel) with
 * ohw_dbg_gemm's contract; N % 64 == 0, K % 64 == 0.  With OHW_GEMM_SMALL=1 (default 0: its on / off times have not been
 * measured yet) run_encode selects it under a reduced audio context when the 128x128 grid would leave more than half the
 * compute units idle; it gives ohw_dbg_gemm's bits.                                                                  */
int ohw_dbg_gemm_small(int dtype, const void* A, const void* W, const float* bias, void* out, int64_t M, int64_t N,
                       int64_t K, int epilogue, void* stream);
int ohw_dbg_attention(int dtype, const void* qkv, void* out, int batch, int T, int n_head, void* stream);
/* The attention kernels on caller data (tests/test_gpu_attn_needles.py).  Large tensors are device pointers of `dtype`, the
 * small integer tables are HOST arrays: each entry checks them, copies them to the device, launches, synchronises the stream
 * and frees its copies.  A table outside the stated ranges is OHW_E_INVALID_ARG before any device work: no launch indexes
 * outside the caller's buffers.
 * ohw_dbg_attention_var: the encoder kernel with per-window lengths.  qkv [rows][3 * 64 * n_head], out [rows][64 * n_head].
 *   win_len [batch], 1 <= win_len[b] <= T: window b attends over its first win_len[b] rows.  win_off null: rows = batch * T,
 *   window b at row b * T; rows of query blocks (128 rows) wholly past win_len[b] are written as zeros, the other rows past it
 *   are unspecified.  win_off [batch], the exclusive prefix sum of win_len: packed rows, window b at row win_off[b], rows = the
 *   sum of the lengths; no other row is stored.  Both null: ohw_dbg_attention.                                               */
int ohw_dbg_attention_var(int dtype, const void* qkv, void* out, int batch, int T, int n_head, const int32_t* win_len_host,
                          const int32_t* win_off_host, void* stream);
/* which kernel a decoder attention launch picked (ohw_dbg_counter's "xattn.*" / "self_attn.*" names, in this order) */
enum { OHW_XA_PLAIN = 0, OHW_XA_SPLIT, OHW_XA_ROWS2, OHW_XA_ROWS3, OHW_XA_ROWS4, OHW_XA_GROUP2, OHW_XA_GROUP3, OHW_XA_GROUP4,
       OHW_XA_GROUP5, OHW_XA_GROUP_SPLIT };
enum { OHW_SA_PLAIN = 0, OHW_SA_SLOTS };
/* ohw_dbg_cross_attn: q [M][d] row-major (d = 64 * n_head); xk / xv head-major [windows][n_head][t_len][64]; out in the decoder
 *   GEMMs' activation-tile order, [ceil(M / 16)][d / 32][64][8] elements: element (m, k) at
 *   ((((m / 16) * (d / 32) + k / 32) * 64 + m % 16 + 16 * ((k % 32) / 8)) * 8) + k % 8; rows >= M are never stored.
 *   Row m reads window m / n_new, or m / kv_group for kv_group = 2 .. 5 beams per window (then n_new = 1); M % n_new == 0 and
 *   M % kv_group == 0.  done [windows] or null: the rows of a window with done != 0 are not stored.  win_len [windows] or null,
 *   1 <= win_len[w] <= t_len: window w's first win_len[w] keys.  partials f32 [max_split_rows][n_head][8][68] and tickets u32
 *   [max_split_rows][n_head] (zero; the kernel leaves them zero), both or neither: scratch of the split forms; with them,
 *   without batch_invariant and win_len, M <= max_split_rows.  *variant_out (may be null): OHW_XA_*.
 * ohw_dbg_self_attn: q [M][d]; k_cache / v_cache [M / n_new][n_head][n_ctx][64]; n_past [M / n_new], 0 <= n_past[b] and
 *   n_past[b] + n_new <= n_ctx: new token i of window b attends over positions 0 .. n_past[b] + i.  kv_slot
 *   [M / n_new][n_ctx] or null, entries in 0 .. M / n_new - 1: the cache row that holds position j of window b's sequence.
 *   out as above.  *variant_out (may be null): OHW_SA_*.                                                                     */
int ohw_dbg_cross_attn(int dtype, const void* q, const void* xk, const void* xv, void* out, int M, int n_new, int n_head, int t_len,
                       int kv_group, int batch_invariant, const int32_t* done_host, const int32_t* win_len_host, float* partials,
                       unsigned* tickets, int max_split_rows, int* variant_out, void* stream);
/* ohw_dbg_cross_attn_chunk: the prefill's cross-attention (cross_attn_chunk_kernel: ohw_state_prefill) on caller data.  q
 *   [windows * 8][d] row-major, row b * 8 + i is query i of window b; xk / xv, win_len and done as above; out in activation-tile
 *   order, ceil(windows * 8 / 16) tiles.  The caller pre-fills out: the rows of a window with done != 0, and the rows of the
 *   last tile past windows * 8, keep what they held.  OHW_E_INVALID_ARG for windows < 1, t_len < 1 and a win_len entry outside
 *   1 .. t_len.                                                                                                             */
int ohw_dbg_cross_attn_chunk(int dtype, const void* q, const void* xk, const void* xv, void* out, int windows, int n_head, int t_len,
                             const int32_t* win_len_host, const int32_t* done_host, void* stream);
/* the same with n_q = 8 or 16 query rows per window (q [windows * n_q][d], row b * n_q + i; out ceil(windows * n_q / 16) tiles);
 * another n_q: OHW_E_INVALID_ARG.  ohw_dbg_cross_attn_chunk is n_q = 8.                                                       */
int ohw_dbg_cross_attn_chunk_n(int dtype, const void* q, const void* xk, const void* xv, void* out, int windows, int n_head, int t_len,
                               const int32_t* win_len_host, const int32_t* done_host, void* stream, int n_q);
int ohw_dbg_self_attn(int dtype, const void* q, const void* k_cache, const void* v_cache, const int32_t* n_past_host, void* out, int M,
                      int n_new, int n_head, int n_ctx, const int32_t* kv_slot_host, int* variant_out, void* stream);
/* The alignment kernels on caller data (tests/test_gpu_align.py).
 * ohw_dbg_align_probs: q [rows][64 * n_head] and xk [n_head][t_len][64] are device pointers of `dtype`, 1 <= rows <= 8,
 *   1 <= n_keys <= t_len; heads [n_heads] (host) picks the heads; p_out [n_heads][rows][t_len] (host): the tap's soft-max over
 *   keys 0 .. n_keys - 1, exactly 0 from n_keys on (those keys are never read).
 * ohw_dbg_align_reduce / ohw_dbg_dtw: the device twins of ohw_align_reduce_host / ohw_dtw_host on host arrays.          */
int ohw_dbg_align_probs(int dtype, const void* q, const void* xk, int rows, int n_head, int t_len, int n_keys,
                        const int32_t* heads_host, int n_heads, float* p_out_host, void* stream);
int ohw_dbg_align_reduce(int device, const float* p_host, int n_heads, int n_all, int n_prompt, int n_keys, float* m_out_host);
int ohw_dbg_dtw(int device, const float* m_host, int n, int n_keys, int32_t* start_idx_out);
/* fill an encoder activation buffer of the state with NaN (every byte 0xff: a NaN in bf16 and in f16): what = "qkv" or "att".
 * An encode overwrites every row it owns, so a test can tell a row that was never written, or written by a neighbour. */
int ohw_dbg_poison(ohw_state* st, const char* what);
/* the detector's kernels alone (vad.hip).  ohw_dbg_vad_energy: vad_band_kernel on pcm (as ohw_state_vad_frames takes it; a
 * device pointer may have samples behind n: they must not count); e_out: HOST array of (n + 159) / 160 + guard floats.
 * ohw_dbg_vad_floor: the floor and probability kernels on a caller's HOST e array of n_frames values (any finite value);
 * prob_out: HOST array of n_frames + guard floats, floor_db_out: one float.  The device output of n_frames + guard floats is
 * filled with OHW_DBG_SENTINEL_F32 (defined below) first and copied back whole: the guard must still hold it.  0 <= guard <= 4096.  */
int ohw_dbg_vad_energy(ohw_state* st, const float* pcm, int64_t n, int pcm_on_device, float* e_out, int guard);
int ohw_dbg_vad_floor(ohw_state* st, const float* e, int64_t n_frames, const ohw_vad_detector* d, float* prob_out, int guard, float* floor_db_out);
/* the DEVICE sampler on caller-supplied rows: logits [batch][n_vocab] (host), history [batch][hist_stride] with
 * n_hist[b] tokens sampled so far in the window.  tokens_out [batch]: the pick (end-of-text included);
 * logprobs_out [batch] / no_speech_out [batch] may be NULL (no-speech is defined for rows with n_hist == 0). */
int ohw_dbg_sample(ohw_state* st, const ohw_sample_params* p, const float* logits, const int32_t* history, int hist_stride,
                   const int32_t* n_hist, int batch, int32_t* tokens_out, float* logprobs_out, float* no_speech_out);
/* the same for the temperature sampler of ohw_sample_pass: temperature > 0, uniforms [batch] the draw of each row's step */
int ohw_dbg_sample_t(ohw_state* st, const ohw_sample_params* p, const float* logits, const int32_t* history, int hist_stride,
                     const int32_t* n_hist, int batch, float temperature, const double* uniforms, int32_t* tokens_out,
                     float* logprobs_out, float* no_speech_out);
/* the group form of that sampler (ohw_sample_pass_n) once on caller data: rows = n_windows * group, row r = candidate r % group
 * of window r / group.  first != 0 (the step behind the prompt): logits [n_windows][n_vocab], every row of a window reads its
 * window's row; first == 0: logits [rows][n_vocab].  history / n_hist / uniforms per row as above; done [rows] in and out: a
 * row with done != 0 is not sampled (token_out 0, nothing written or advanced).  win_done_out [n_windows]: 1 once every row of
 * the window is done - the windows whose rows all came in done start at 1, the others are set by the row that finishes last.
 * n_cur_out [rows] (may be NULL): tokens in the row's history afterwards.  The other outputs as above.                     */
int ohw_dbg_sample_group(ohw_state* st, const ohw_sample_params* p, const float* logits, const int32_t* history, int hist_stride,
                         const int32_t* n_hist, int n_windows, int group, int first, float temperature, const double* uniforms,
                         int32_t* done, int32_t* tokens_out, float* logprobs_out, float* no_speech_out, int32_t* win_done_out,
                         int32_t* n_cur_out);
/* the DEVICE language pick (ohw_state_detect_window_lang's kernel) on caller-supplied rows: logits [batch][n_vocab] (host);
 * ids_out [batch], probs_out [batch][n_langs] or NULL.  Leaves the state's language table alone.                       */
int ohw_dbg_lang_pick(ohw_state* st, const float* logits, int batch, int32_t* ids_out, float* probs_out);
/* counters of a state's three graph caches, one cache type with capacities 8 (step: ohw_greedy*, ohw_sample_pass), 4 (group:
 * ohw_sample_pass_n) and 4 pairs (beam: ohw_beam_search*), the oldest entry evicted: "step_captures" / "beam_captures" (entries
 * captured so far by the step and the group cache together / by the beam cache, a pair counting once), "step_graphs" /
 * "group_graphs" / "beam_graphs" (entries held now), "persist_launches" (persistent decoder steps launched or captured),
 * "enc_rows" (rows M of the dense encoder GEMMs of the last encode: B * E, or the sum of the lengths when it ran packed);
 * OHW_E_INVALID_ARG for another name.  A second ohw_greedy /
 * ohw_beam_search with the same batch, parameters and stream must add no capture (tests/test_gpu_beam.py).
 * The decoder step's kernel variants, launches counted per state since its creation (host-side: a captured step
 * counts once, at its capture; saturates at INT32_MAX):
 *   "dec_gemm.<gemm><form>.<NT>x<MT>"  gemm: qkv, o (self-attention out), xq, xo (cross-attention q / out), fc1, fc2,
 *                                      logits; form: ".ln" (LayerNorm in the prologue), ".pn" (post-norm), ".ks"
 *                                      (split-K), "" (none); NT x MT n-tiles x m-tiles per workgroup: 1x1 2x1 1x2 2x2 4x2 1x6,
 *                                      4x6 5x6 (qkv.ln, fc1.ln: all rows behind a LayerNorm launch of its own; logits: 4x6,
 *                                      all rows, on a CU-masked stream)
 *   "xattn.plain" / "xattn.split"      cross-attention, one workgroup per (row, head) / keys cut over gridDim.z > 1
 *   "xattn.rows2" .. "xattn.rows4"     one workgroup per (window, head) for 2..4 new tokens
 *   "xattn.chunk"                      the prefill's 8 rows per window on the MFMA units (ohw_state_prefill)
 *   "xattn.group2" .. "xattn.group5"   the same for 2..5 beams of a window; "xattn.group_split": beams, keys cut
 *   "self_attn.plain" / ".slots"       masked self-attention, without / with the beam kv_slot table; ".fused" /
 *                                      ".fused_slots": the same inside the QKV launch (OHW_DEC_FUSE_ATTN=1)
 *   "phrase_boost"                     launches of the hot-phrase kernel (ohw_state_set_phrase_table); 0 with no table
 *   "repeat_rule"                      launches of the repetition kernel (ohw_state_set_repeat_rule); 0 while the rule is off
 *   "command_rule"                     launches of the command-list kernel (ohw_state_set_command_table); 0 with no list
 *   "dec_gemm.total" / "xattn.total"   the sum over every "dec_gemm.*" / "xattn.*" name above ("xattn.chunk" is not in it)
 *   "token_score"                      launches of token_score_kernel (ohw_state_score): one per replay chunk
 *   "score_buffers"                    1 while the state holds ohw_state_score's buffers, else 0
 * The persistent step (ohw_state_set_persistent) counts only its logits GEMM.                                    */
int ohw_dbg_counter(const ohw_state* st, const char* name);

/* ONE beam step (beam_topk_kernel + beam_update_kernel, as ohw_beam_search launches them) on caller-supplied host data; the
 * whole resulting state comes back.  No decoder runs.  Rows: beam j of window w is row w * K + j, R = W * K rows.
 * side (0 / 1): which half of the token-history and kv_slot double buffers holds the input; the step writes the other half,
 * as ohw_beam_search alternates them.  The state's logit bias applies; p->n_max is used as given (not clamped).
 * Every range is checked on the host before any device work (OHW_E_INVALID_ARG): K in 2..5, R <= max_batch,
 * 0 <= n_cur[w] < n_text_ctx (the state's token capacity), 0 <= n_past_w[w] and n_past_w[w] + 2 <= n_text_ctx,
 * fin_cnt[w] in 0..K, fin_len of the used pool slots in 0..n_text_ctx, history tokens (the first n_cur[w] of a row) in
 * 0..n_vocab - 1 and, when first == 0, the kv_slot entries of positions 0..n_past_w[w] in 0..R - 1 (of a window with win_done
 * set only fin_cnt and fin_len are checked: the kernels read nothing else of it).
 * Before the launch tokens_next, kv_slot_next, cand_tok / cand_lp, next_tok, n_past and the pool slots from fin_cnt[w] on
 * are filled with OHW_DBG_SENTINEL_I32 / OHW_DBG_SENTINEL_F32 and then copied back whole: what holds the sentinel afterwards
 * was not written.  tickets_out: the top-k's ticket words, zero after every launch.  A later ohw_beam_search on the state
 * is not disturbed (it re-initialises what it uses). */
#define OHW_DBG_SENTINEL_I32 (-7777777)
#define OHW_DBG_SENTINEL_F32 (-12345.0f)
typedef struct {
  int32_t first, K, W, side;
  const float* logits;     /* in  [first ? W : R][n_vocab] */
  const int32_t* tokens;   /* in  [R][n_text_ctx] token histories, n_cur[w] of them used per row */
  const int32_t* kv_slot;  /* in  [R][n_text_ctx] */
  int32_t* n_cur;          /* in / out [W] */
  int32_t* n_past_w;       /* in / out [W] position the step that just ran wrote */
  int32_t* win_done;       /* in / out [W] */
  float* beam_sum;         /* in / out [R] */
  int32_t* fin_cnt;        /* in / out [W] */
  int32_t* fin_tok;        /* in / out [R][n_text_ctx] */
  int32_t* fin_len;        /* in / out [R] */
  float* fin_sum;          /* in / out [R] */
  int32_t* cand_tok;       /* out [R][K + 1] */
  float* cand_lp;          /* out [R][K + 1] */
  int32_t* tokens_next;    /* out [R][n_text_ctx] */
  int32_t* kv_slot_next;   /* out [R][n_text_ctx] */
  int32_t* next_tok;       /* out [R] */
  int32_t* n_past;         /* out [R] */
  int32_t* n_done;         /* out [1] windows that finished in this step */
  uint32_t* tickets_out;   /* out [R] */
} ohw_dbg_beam_io;
int ohw_dbg_beam_step(ohw_state* st, const ohw_sample_params* p, const ohw_dbg_beam_io* io);

/* ohw_dbg_beam_step with the log-probability history and the no-speech probability of ohw_beam_search_ex.  base: as above.
 * plog NULL: the kernels touch no history (plog_next and fin_plog are then left alone) and the call is ohw_dbg_beam_step.
 * Otherwise plog_next is filled with OHW_DBG_SENTINEL_F32 before the launch, as are fin_plog's rows from fin_cnt[w] on, and
 * both come back whole.  nosp_prob (or NULL): sentinel-filled; written for the windows of a first step only.               */
typedef struct {
  ohw_dbg_beam_io base;
  const float* plog;       /* in  [R][n_text_ctx + 1] or NULL: log-probability of every history token, n_cur[w] used per row */
  float* plog_next;        /* out [R][n_text_ctx + 1] */
  float* fin_plog;         /* in / out [R][n_text_ctx + 1]: fin_len values per used pool slot, end-of-text's at index fin_len */
  float* nosp_prob;        /* out [W] or NULL */
} ohw_dbg_beam_io_ex;
int ohw_dbg_beam_step_ex(ohw_state* st, const ohw_sample_params* p, const ohw_dbg_beam_io_ex* io);

/* ONE sampler launch (temperature == 0: sampler_kernel as ohw_greedy launches it; > 0: sampler_t_kernel as ohw_sample_pass
 * does) on caller-supplied host rows, and the sampler's WHOLE output: what ohw_dbg_sample / ohw_dbg_sample_t leave out (the
 * history rows, the counters, the finishing flags, the log-probability rows, the ticket words).  No decoder runs; the state's
 * logit bias applies; p->n_max and p->force_len are used as given.  M = the state's token capacity (n_text_ctx).
 * Every range is checked on the host before any device work (OHW_E_INVALID_ARG): batch in 1..max_batch, advance 0 or 1,
 * temperature >= 0 (uniforms not NULL and in [0, 1) when > 0), 0 <= n_cur[b] < M, 0 <= n_past[b] and
 * n_past[b] + advance < n_text_ctx, the first n_cur[b] tokens of a row in 0..n_vocab - 1.
 * Before the launch next_tok, tok_lp, nosp_prob and the history slot at n_cur[b] of every row are filled with
 * OHW_DBG_SENTINEL_I32 / OHW_DBG_SENTINEL_F32; afterwards everything is copied back whole: what holds the sentinel was not
 * written.  tickets_out: the sampler's ticket words, zero after every launch.                                             */
typedef struct {
  int32_t batch, advance;
  float temperature;
  const float* logits;     /* in  [batch][n_vocab] */
  const double* uniforms;  /* in  [batch] the draw of each row's step, or NULL when temperature == 0 */
  int32_t* tokens;         /* in / out [batch][M] token histories, n_cur[b] of them used */
  int32_t* n_cur;          /* in / out [batch] */
  int32_t* n_past;         /* in / out [batch] */
  int32_t* done;           /* in / out [batch]: a row that comes in done is not touched */
  float* sum_logprob;      /* in / out [batch] */
  int32_t* next_tok;       /* out [batch] */
  float* tok_lp;           /* out [batch][M + 1] */
  float* nosp_prob;        /* out [batch]: written for rows with n_cur == 0 */
  int32_t* n_done;         /* out [1] rows that finished in this launch */
  uint32_t* tickets_out;   /* out [batch] */
} ohw_dbg_sample_io;
int ohw_dbg_sample_ex(ohw_state* st, const ohw_sample_params* p, const ohw_dbg_sample_io* io);

/* the final ranking of a beam search on caller-supplied pool and live state (host arrays), R = W * K rows:
 * candidates are window w's pool entries 0 .. fin_cnt[w] - 1 in pool order; if fewer than K, its live beams join by
 * descending beam_sum (equal sums: the lower beam index; -inf skipped) until there are K; score = sum / max(1, n) in fp32
 * with a correctly rounded division; the first strict maximum wins.  Written per window: the winner's first
 * min(n, max_tokens) tokens and log-probabilities, end-of-text's log-probability after them when it came from the pool
 * (ended_by_eot = 1), n_tokens, sum_logprob, n_finished = fin_cnt[w]; a window without any candidate gives n_tokens 0,
 * sum_logprob 0, ended_by_eot 0.  Checked first (OHW_E_INVALID_ARG): K in 2..5, W >= 1, 1 <= stride, 0 <= max_tokens <= stride,
 * fin_cnt in 0..K, fin_len of the used slots and n_cur in 0..stride.
 * ohw_dbg_beam_finish runs beam_finish_kernel (needs W * K <= max_batch and stride == n_text_ctx, the state's token capacity);
 * out_tokens / out_logprobs / n_tokens / sum_logprob / ended_by_eot / n_finished are filled with the sentinels first, so what
 * the kernel did not write shows.  ohw_beam_finish_host is the same rule on the host, no GPU, with the same sentinel fill.  */
typedef struct {
  int32_t K, W, stride, max_tokens;
  const int32_t* fin_cnt;  /* [W] */
  const int32_t* fin_len;  /* [R] */
  const float* fin_sum;    /* [R] */
  const int32_t* fin_tok;  /* [R][stride] */
  const float* fin_plog;   /* [R][stride + 1] */
  const int32_t* n_cur;    /* [W] length of every live beam */
  const int32_t* tokens;   /* [R][stride] live histories */
  const float* plog;       /* [R][stride + 1] */
  const float* beam_sum;   /* [R] */
  int32_t* out_tokens;     /* out [W][max_tokens] */
  float* out_logprobs;     /* out [W][max_tokens + 1] */
  int32_t* n_tokens;       /* out [W] */
  float* sum_logprob;      /* out [W] */
  int32_t* ended_by_eot;   /* out [W] */
  int32_t* n_finished;     /* out [W] */
} ohw_beam_finish_io;
int ohw_dbg_beam_finish(ohw_state* st, const ohw_beam_finish_io* io);
int ohw_beam_finish_host(const ohw_beam_finish_io* io);

/* ONE decoder GEMM launch (launch_dec_gemm: decode.hip) on caller data (tests/test_gpu_dec_gemm.py); no ohw_state.  Every
 * pointer but n_past is a DEVICE pointer; the entry checks every range on the host before any device work (OHW_E_INVALID_ARG,
 * nothing launched), prepares the weights on private copies with the loader's own kernels, launches once on `stream`,
 * synchronises it and frees its copies.
 * Weights: w f32 [N][K] row-major, bias f32 [N] or NULL, gamma / beta f32 [K], both or neither: with them the LayerNorm's
 *   affine part is folded first (launch_fold_ln: bias += W beta, W *= gamma; a NULL bias counts as zeros), then the matrix is
 *   rounded to `dtype` in fragment-tile order with ceil16(N) rows (launch_repack_tiled), and for form PN its row sums are
 *   taken (launch_tiled_rowsum).
 * Activations, by form:
 *   PLAIN  x: `dtype` activation tiles [ceil(M / 16)][K / 32][64][8] (the order ohw_dbg_cross_attn documents for its output)
 *   LN     x: f32 [M][K]; (x - mean) * rstd is fused into the prologue; K % 64 == 0, K <= 1280; epilogues QKV, BIAS_T, GELU_T
 *   PN     x: tiles as PLAIN, stat_in f32 [M][K / 16][2] (mean and sum of squared deviations of 16 columns):
 *          out = rstd * (x W^T - mean * wsum) + bias; K / 16 <= 128 statistics tiles; epilogues QKV, BIAS_T, GELU_T
 * Epilogues (M rows, out written for rows < M and columns < N only):
 *   QKV     N == 3 * d_model, d_model == 64 * n_head, M % n_new == 0.  out: `dtype` [M][d_model] (q, ld_out ignored);
 *           k_cache / v_cache `dtype` [M / n_new][n_head][n_ctx][64]: row m = b * n_new + i stores position n_past[b] + i, and
 *           nothing when that is >= n_ctx.  n_past: HOST [M / n_new], 0 <= n_past[b] <= n_ctx
 *   BIAS_T  out `dtype` [M][ld_out]            GELU_T  out `dtype` activation tiles [ceil(M / 16)][N / 32][64][8], N % 32 == 0
 *   RESID   out f32 [M][ld_out] += x W^T + bias.  ksplit > 1 (form PLAIN): K cut over ksplit workgroups per tile,
 *           2 <= ksplit <= K / 32, slab f32 of slab_bytes >= ceil(N / 16) * ceil(M / 32) * ksplit * 2048 bytes, ticket u32
 *           [ceil(N / 16) * ceil(M / 32)] zero before and after.  x16_out and stat_out (both or neither; form PLAIN, no
 *           split, N % 32 == 0): also the `dtype` tiled copy [ceil(M / 16)][N / 32][64][8] of the new rows and f32
 *           [M][N / 16][2] statistics of every 16 columns
 *   LOGITS  out f32 [M / n_new][ld_out]: only rows m with m % n_new == n_new - 1 are stored, as row m / n_new
 *   ld_out >= N wherever it is used.  cu_budget: compute units the launch may use (0: the whole device); with M, N and K it
 *   decides the work shape.  *shape_out (may be NULL): OHW_DG_SHAPE_* of the kernel that ran. */
enum { OHW_DEPI_QKV = 0, OHW_DEPI_BIAS_T, OHW_DEPI_BIAS_GELU_T, OHW_DEPI_BIAS_RESID, OHW_DEPI_LOGITS };
enum { OHW_DG_FORM_PLAIN = 0, OHW_DG_FORM_LN, OHW_DG_FORM_PN };
enum { OHW_DG_SHAPE_1x1 = 0, OHW_DG_SHAPE_2x1, OHW_DG_SHAPE_1x2, OHW_DG_SHAPE_2x2, OHW_DG_SHAPE_4x2, OHW_DG_SHAPE_1x6,
       OHW_DG_SHAPE_4x6, OHW_DG_SHAPE_5x6 };
typedef struct {
  int32_t dtype, epilogue, form;
  int32_t M, N, K, n_new;
  int64_t ld_out;
  int32_t cu_budget, ksplit;
  const float* w;          /* f32 [N][K] */
  const float* bias;       /* f32 [N] or NULL */
  const float* gamma;      /* f32 [K] or NULL */
  const float* beta;       /* f32 [K] or NULL */
  const void* x;
  const float* stat_in;    /* form PN */
  void* out;
  float* slab;             /* ksplit > 1 */
  int64_t slab_bytes;
  uint32_t* ticket;
  void* x16_out;           /* RESID producer, or NULL */
  float* stat_out;
  void* k_cache;           /* QKV */
  void* v_cache;
  const int32_t* n_past;   /* QKV: HOST [M / n_new] */
  int32_t d_model, n_head, n_ctx;
  int32_t* shape_out;      /* HOST, or NULL */
} ohw_dbg_dec_gemm_io;
int ohw_dbg_dec_gemm(const ohw_dbg_dec_gemm_io* io, void* stream);
/* ohw_dbg_dec_gemm with epilogue LOGITS (anything else: OHW_E_INVALID_ARG) plus the all-rows output ohw_state_score's replay
 * uses: out_all DEVICE f32 [M][ld_all], ld_all >= N - every row m < M, column n < N is stored at out_all[m * ld_all + n],
 * nothing else; g.out is written as ever.  out_all == NULL: the launch ohw_dbg_dec_gemm makes (the work shape never depends on
 * out_all). */
typedef struct { ohw_dbg_dec_gemm_io g; float* out_all; int64_t ld_all; } ohw_dbg_logits_rows_io;
int ohw_dbg_logits_rows(const ohw_dbg_logits_rows_io* io, void* stream);
/* token_score_kernel once on caller data (tests/test_gpu_token_score.py), on the state's device and stream; the state's own
 * buffers are not touched.  logits HOST f32 [batch * 8][ld] (ld % 4 == 0, ld >= n_vocab; the caller poisons the padding columns):
 * staged on the device between two guard rows of NaN, which the kernel must never read into a result.  targets HOST [batch * 8]
 * (0 .. n_vocab - 1), n_all HOST [batch], row0 >= 0, n_prompt >= 1, cap >= 1: TokenScoreParams of kernels.hpp, that is row
 * m = b * 8 + j writes entry row0 + j - (n_prompt - 1) of window b iff n_prompt - 1 <= row0 + j < n_all[b] and the entry is
 * below cap.  out HOST [guard + batch * cap + guard] entries: the device copy is filled with OHW_DBG_SENTINEL_F32 (top_id:
 * OHW_DBG_SENTINEL_I32) first and copied back whole, the guards in front and behind included: what holds the sentinel afterwards
 * was not written.  0 <= guard <= 4096, batch <= 4096, n_vocab <= 2^20. */
int ohw_dbg_token_score(ohw_state* st, const float* logits, int batch, int64_t ld, int n_vocab, int eot, const int32_t* targets,
                        const int32_t* n_all, int row0, int n_prompt, int cap, int guard, ohw_token_score* out);
/* launch_embed on caller data: emb f32 [n_vocab][d] (device; rounded and tiled like a weight matrix, rows padded to a multiple
 * of 16), pos f32 [n_pos][d] (device), tok and n_past HOST tables [M] and [M / n_new]: 0 <= tok[m] < n_vocab,
 * 0 <= n_past[b] and n_past[b] + n_new <= n_pos; M % n_new == 0, d % 32 == 0.  x f32 [M][d] = emb[tok[m]] + pos[n_past[m / n_new]
 * + m % n_new]; x16 (`dtype` tiles [ceil(M / 16)][d / 32][64][8]) and stat (f32 [M][d / 16][2]) may be NULL. */
int ohw_dbg_embed(int dtype, const float* emb, int n_vocab, const float* pos, int n_pos, const int32_t* tok_host,
                  const int32_t* n_past_host, float* x, void* x16, float* stat, int M, int n_new, int d, void* stream);
/* launch_layernorm on caller data (device pointers): x f32 [rows][d], gamma / beta f32 [d]; y `dtype` [rows][d] row-major, or
 * with tiled != 0 activation tiles [ceil(rows / 16)][d / 32][64][8] (then d % 32 == 0).  d % 4 == 0, 4 <= d <= 2048. */
int ohw_dbg_layernorm(int dtype, const float* x, const float* gamma, const float* beta, void* y, int64_t rows, int d, int tiled,
                      void* stream);

/* ONE encoder GEMM launch (gemm.hip 128x128, gemm256.hip 256x256, gemm_small.hip 64x64) on caller data, in any of the forms
 * run_encode launches (tests/test_gpu_enc_gemm.py); no ohw_state.  a, w, bias, pos and out are DEVICE pointers, c_row_map is a
 * HOST table.  Every range is checked on the host before any device work (OHW_E_INVALID_ARG, nothing launched); then the
 * weights are prepared on a private copy with the loader's own kernels, the GEMM is launched once on `stream`, the stream is
 * synchronised and the copies are freed.
 * Geometry: gemm.hpp's GemmParams.  Row m of A is at a + (m / rows_per_batch) * a_batch_stride + (m % rows_per_batch) * lda
 *   and has K elements of `dtype` (rows may overlap: lda < K); with nb = ceil(M / rows_per_batch) windows,
 *   (nb - 1) * a_batch_stride + (min(M, rows_per_batch) - 1) * lda + K <= a_elems.  K % 64 == 0; lda and a_batch_stride are
 *   multiples of 8 elements and a is 16-byte aligned.
 * Weights: w f32 [N][K] row-major, rounded to `dtype` (launch_convert_rows); with conv_cin > 0 w is a convolution's f32
 *   [N][conv_cin][3] instead and is repacked tap-major with c_pad = K / 3 zero-padded channels (launch_repack_conv: K % 3 == 0,
 *   conv_cin <= K / 3).  bias f32 [N] or NULL.
 * Epilogues (gemm.hpp's GemmEpilogue, 0 .. 5):
 *   0 BIAS_T, 1 BIAS_GELU_T       out `dtype`; 2 BIAS_RESID_F32 (out +=), 3 GELU_POS_F32 (+ pos[m % rows_per_batch][n], pos f32
 *   [rows_per_batch][N]), 4 F32   out f32.  Row m goes to out + (m / rows_per_batch) * c_batch_stride + (m % rows_per_batch) * ldc,
 *       N elements; ldc >= N, windows must not overlap (c_batch_stride >= (min(M, rows_per_batch) - 1) * ldc + N when nb > 1),
 *       (nb - 1) * c_batch_stride + (min(M, rows_per_batch) - 1) * ldc + N <= out_elems; ldc and c_batch_stride are multiples
 *       of 16 bytes, out is 16-byte aligned.
 *   5 CROSSKV_T                   out `dtype` head-major [N / d_model][batch][n_head][t_len][64]: column n = slab * d_model + 64 h + dh
 *       of row m goes to [slab][batch_offset + m / rows_per_batch][h][m % rows_per_batch][dh]; d_model == 64 * n_head,
 *       N % d_model == 0, min(M, rows_per_batch) <= t_len, 0 <= batch_offset, batch_offset + nb <= batch,
 *       N / d_model * batch * n_head * t_len * 64 <= out_elems.  c_row_map (HOST [M], epilogue 5 only) or NULL: with it row m
 *       goes to window batch_offset + c_row_map[m] / t_len, position c_row_map[m] % t_len, whatever rows_per_batch is;
 *       0 <= c_row_map[m] <= (batch - batch_offset) * t_len - 1.
 * kernel: AUTO is launch_gemm's own pick; K128 needs N % 128 == 0, SMALL N % 64 == 0, K256 N % 256 == 0. */
enum { OHW_EG_KERNEL_AUTO = 0, OHW_EG_KERNEL_K128, OHW_EG_KERNEL_SMALL, OHW_EG_KERNEL_K256 };
typedef struct {
  int32_t dtype, epilogue, kernel;
  int32_t conv_cin;            /* > 0: w is [N][conv_cin][3] */
  int64_t M, N, K;
  int64_t lda, a_batch_stride, rows_per_batch;
  int64_t ldc, c_batch_stride;
  int32_t d_model, n_head, t_len, batch, batch_offset;   /* CROSSKV_T */
  const int32_t* c_row_map;    /* HOST [M] or NULL */
  const void* a;
  int64_t a_elems;
  const float* w;
  const float* bias;           /* f32 [N] or NULL */
  const float* pos;            /* GELU_POS_F32 */
  void* out;
  int64_t out_elems;
} ohw_dbg_enc_gemm_io;
int ohw_dbg_enc_gemm(const ohw_dbg_enc_gemm_io* io, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OHW_H */
