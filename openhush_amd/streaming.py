"""Streaming glue around the path (BASELINE.json config #5): the daemon's chunk scheduler in front of the
engine and the TranscriptionTracker behind it, host side.

    ChunkScheduler     <- the chunk-timer arm of the daemon loop (reference src/daemon.rs:1912-2013) + AudioRecorder::
                          extract_chunk (src/input/audio.rs:741-776): on every tick the audio since the last tick becomes a job
                          (dropped below 0.1 s, padded to 1.1 s), registered with the tracker under its back-pressure settings
    StreamingSession   ties it to the MI355X path: an optional VAD gate (reference VadEngine hook: chunks without speech are
                          not decoded), one 30 s window per chunk through mel -> encoder -> beam search (beam = 5, the
                          hipGraph-captured decoder step) or the greedy loop, detokenise, tracker.add_result ->
                          take_ready (overlap de-duplication and ordering are the tracker's)
Nothing here computes: the arithmetic is in libohw.so.
"""
from __future__ import annotations

import dataclasses
from typing import Callable, List, Optional

import numpy as np

from . import engine as E
from .tracker import BackpressureStrategy, ChunkResult, TranscriptionTracker

SAMPLE_RATE = 16000
MIN_DURATION_SECS = 0.1            # reference src/input/audio.rs:29
WHISPER_MIN_DURATION_SECS = 1.1    # reference src/input/audio.rs:34


@dataclasses.dataclass
class ChunkJob:
    """reference src/queue/mod.rs TranscriptionJob"""
    samples: np.ndarray
    sequence_id: int
    chunk_id: int
    is_final: bool = False


def extract_chunk(recording: np.ndarray, from_pos: int, to_pos: int) -> Optional[np.ndarray]:
    """AudioRecorder::extract_chunk for a 16 kHz recorder: None below 0.1 s, zero-padded to 1.1 s (17 600 samples)"""
    s = np.asarray(recording[from_pos:to_pos], dtype=np.float32)
    if s.size == 0 or s.size / SAMPLE_RATE < MIN_DURATION_SECS:
        return None
    need = int(SAMPLE_RATE * WHISPER_MIN_DURATION_SECS)
    if s.size / SAMPLE_RATE < WHISPER_MIN_DURATION_SECS:
        s = np.concatenate([s, np.zeros(need - s.size, np.float32)])
    return s


class ChunkScheduler:
    """One recording (sequence): tick(current_pos) returns the job for the audio since the last tick, or None (too short, or
    refused by the tracker's back-pressure - the position still advances, as in the reference)."""

    def __init__(self, tracker: TranscriptionTracker, sequence_id: int, max_pending: int = 10, high_water_mark: int = 8,
                 strategy: BackpressureStrategy = BackpressureStrategy.WARN):
        self.tracker, self.sequence_id = tracker, sequence_id
        self.max_pending, self.high_water_mark, self.strategy = max_pending, high_water_mark, strategy
        self.last_chunk_pos = 0
        self.next_chunk_id = 0
        self.rejected = 0

    def tick(self, recording: np.ndarray, current_pos: int, is_final: bool = False) -> Optional[ChunkJob]:
        buf = extract_chunk(recording, self.last_chunk_pos, current_pos)
        if buf is None:
            return None                                   # "Chunk too short, skipping": the position is kept
        accepted = self.tracker.add_pending_with_config(self.sequence_id, self.next_chunk_id, self.max_pending, self.high_water_mark,
                                                        self.strategy)
        job = ChunkJob(buf, self.sequence_id, self.next_chunk_id, is_final) if accepted else None
        if not accepted:
            self.rejected += 1
        self.last_chunk_pos = current_pos
        self.next_chunk_id += 1
        return job


class NativeChunkScheduler:
    """The scheduler behind the C ABI (ohw_chunk_scheduler_*, csrc/tracker.cpp) on a NativeTranscriptionTracker; same
    interface and behaviour as ChunkScheduler."""
    def __init__(self, tracker, sequence_id: int, max_pending: int = 10, high_water_mark: int = 8,
                 strategy: BackpressureStrategy = BackpressureStrategy.WARN):
        import ctypes as C
        from .tracker import _STRATEGY_CODE
        self._C, self._L = C, E.lib()
        self.tracker, self.sequence_id = tracker, sequence_id
        self.h = C.c_void_p(self._L.ohw_chunk_scheduler_new(tracker.h, sequence_id, max_pending, high_water_mark, _STRATEGY_CODE[strategy]))
        if not self.h:
            raise ValueError("ohw_chunk_scheduler_new")

    last_chunk_pos = property(lambda self: int(self._L.ohw_chunk_scheduler_position(self.h)))
    next_chunk_id = property(lambda self: int(self._L.ohw_chunk_scheduler_next_id(self.h)))
    rejected = property(lambda self: int(self._L.ohw_chunk_scheduler_rejected(self.h)))

    def tick(self, recording: np.ndarray, current_pos: int, is_final: bool = False) -> Optional[ChunkJob]:
        C = self._C
        rec = np.ascontiguousarray(recording, dtype=np.float32)
        fp = C.POINTER(C.c_float)
        cid, frm = C.c_uint32(), C.c_int64()
        n = int(self._L.ohw_chunk_scheduler_tick(self.h, rec.ctypes.data_as(fp), rec.size, current_pos, C.byref(cid), C.byref(frm)))
        if n < 0:
            raise ValueError("ohw_chunk_scheduler_tick")
        if n == 0:
            return None
        buf = np.empty(n, np.float32)
        self._L.ohw_extract_chunk(rec.ctypes.data_as(fp), rec.size, frm.value, current_pos, buf.ctypes.data_as(fp), n)
        return ChunkJob(buf, self.sequence_id, int(cid.value), is_final)

    def close(self):
        if self.h:
            self._L.ohw_chunk_scheduler_free(self.h)
            self.h = self._C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001 - interpreter shutdown
            pass


def native_extract_chunk(recording: np.ndarray, from_pos: int, to_pos: int) -> Optional[np.ndarray]:
    """ohw_extract_chunk"""
    import ctypes as C
    rec = np.ascontiguousarray(recording, dtype=np.float32)
    fp = C.POINTER(C.c_float)
    n = int(E.lib().ohw_extract_chunk(rec.ctypes.data_as(fp), rec.size, from_pos, to_pos, C.cast(None, fp), 0))
    if n <= 0:
        return None
    out = np.empty(n, np.float32)
    E.lib().ohw_extract_chunk(rec.ctypes.data_as(fp), rec.size, from_pos, to_pos, out.ctypes.data_as(fp), n)
    return out


class StreamingSession:
    """Chunks of one recording through the MI355X path, in the worker's stage order (reference src/queue/worker.rs:119-193):
    noise reduction (the RNNoise stage of BASELINE config #5: a plugged-in `denoiser`, reference src/input/audio.rs:249-341) ->
    normalise / compress / limit when `audio_config.preprocessing` is on (:196-240) -> VAD gate -> every 30 s window of the
    job through mel -> encoder -> beam search or greedy -> text.  beam_size 0 = greedy; vad: callable samples -> probability
    (the VadEngine hook) with `vad_threshold`, or None.  audio_ctx: 0 (default) the full 30 s context, n a fixed reduced
    context (a window with samples past n * 320 is refused), "auto" engine.audio_ctx_for(len) for a job of at most one window -
    a 1.1 s chunk then pays for 128 encoder positions instead of 1500 (WhisperEngine.set_audio_ctx's rule).  hot_phrases: terms
    whose continuation is raised while a window's own tokens end in their front part (WhisperEngine.set_hot_phrases).
    repetition_penalty / no_repeat_ngram_size: the two controls of WhisperEngine.set_repetition on the session's state; the
    defaults (1.0, 0) are off.  commands / command_penalty: a closed list of phrases every chunk is held to
    (WhisperEngine.set_commands's rule on the session's state); after a chunk, last_command is the index of the phrase its tokens
    were, or -1, and last_list_logprob the log-probability that the unconstrained model starts a listed phrase.  confidence:
    every window's text tokens are scored by the unconstrained model on the session's state (State.score) and the chunk's
    ChunkResult carries token_probs and word_probs (WhisperEngine.set_confidence's definitions; logprob_decode is NaN here: the
    session's decodes do not return per-token log-probabilities)."""

    def __init__(self, ctx: E.Context, beam_size: int = 5, vad: Optional[Callable[[np.ndarray], float]] = None, vad_threshold: float = 0.5,
                 sequence_id: int = 1, tracker: Optional[TranscriptionTracker] = None, params: Optional[E.SampleParams] = None,
                 audio_config: Optional[E.PreprocessConfig] = None, noise_reduction: bool = False, noise_reduction_strength: float = 1.0,
                 denoiser: Optional["E.Denoiser"] = None, audio_ctx=0, carry_context: bool = False, hot_phrases=None, hot_phrase_boost=1.0,
                 repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0, commands=None, command_penalty: float = E.COMMAND_PENALTY_DEFAULT,
                 confidence: bool = False):
        self.ctx = ctx
        self.confidence = bool(confidence)
        self.audio_ctx = E._audio_ctx_arg(audio_ctx)
        if self.audio_ctx > ctx.hp.n_audio_ctx:
            raise E.WhisperError(E.OHW_E_INVALID_ARG, f"audio_ctx {self.audio_ctx} exceeds the model's {ctx.hp.n_audio_ctx}")
        self.beam_size = beam_size
        self.state = E.State(ctx, max(1, beam_size))          # one window at a time: beam_size decoder rows
        self.vad, self.vad_threshold = vad, vad_threshold
        self.tracker = tracker or TranscriptionTracker()
        self.scheduler = ChunkScheduler(self.tracker, sequence_id)
        self.params = params or ctx.default_params()
        self.audio_config = audio_config
        self.noise_reduction, self.noise_reduction_strength, self.denoiser = noise_reduction, noise_reduction_strength, denoiser
        if noise_reduction and denoiser is None:
            raise E.WhisperError(E.OHW_E_INVALID_ARG, "noise reduction is enabled but no denoise engine is plugged in")
        self.skipped_silent = 0
        self.windows_decoded = 0
        # carry_context: the text tokens of the window just decoded are the next window's context (ohw_state_set_window_prompt),
        # clipped to the last n_text_ctx / 2 - 1; carried across the jobs of the session, reset by a job the VAD skips
        self.carry_context = carry_context
        self.context: List[int] = []
        # hot_phrases: strings (each in its two tokenisations) or token-id lists, raised by hot_phrase_boost - one value, or one
        # per phrase - on the session's state (WhisperEngine.set_hot_phrases's rule, State.set_phrase_table)
        if hot_phrases:
            self.state.set_phrase_table(*E.hot_phrase_tokens(ctx, hot_phrases, hot_phrase_boost))
        if repetition_penalty != 1.0 or no_repeat_ngram_size != 0:
            self.state.set_repeat_rule(repetition_penalty, no_repeat_ngram_size)
        self.last_command, self.last_list_logprob = -1, float("nan")
        self._command_table, self._command_index = None, []
        if commands:
            toks, self._command_index = E.command_tokens(ctx, commands)
            self.state.set_command_table(toks, E.command_penalty_arg(command_penalty))
            self._command_table = E.command_table_build_host(toks, int(ctx.tok.eot))

    def _text(self, tokens: List[int]) -> str:
        return b"".join(self.ctx.token_text(t) for t in tokens if t < self.ctx.tok.eot).decode("utf-8", "replace").strip()

    def _score_window(self, toks, window: int, text0: int, token_probs: list, word_probs: list):
        """State.score on the window just decoded (its cross K/V is resident): the engine's token and word records"""
        text_toks = [int(t) for t in toks if t < self.ctx.tok.eot][:self.ctx.hp.n_text_ctx // 2]
        if not text_toks:
            return
        sc = self.state.score([text_toks], p=self.params)[0]
        tb = [self.ctx.token_text(t) for t in text_toks]
        lpt = []
        for t, s in zip(text_toks, sc[:-1]):
            lt, la, tt = E.token_prob_host(s)
            lpt.append(lt)
            token_probs.append({"id": t, "window": window, "logprob_text": float(lt), "logprob_all": float(la), "logprob_decode": float("nan"),
                                "top_id": int(s["top_id"]), "top_logprob_text": float(tt)})
        starts = E.word_starts(tb)
        probs = E.word_probs_host(lpt, [int(x) for x in starts])
        off, k = text0, -1
        for i, b in enumerate(tb):
            if i == 0 or starts[i]:
                k += 1
                word_probs.append({"text": "", "text_off": off, "text_len": 0, "probability": float(probs[k])})
            w = word_probs[-1]
            w["text_len"] = off + len(b) - w["text_off"]
            off += len(b)
        for w in word_probs:
            if not w["text"]:
                w["text"] = b"".join(tb)[w["text_off"] - text0:w["text_off"] - text0 + w["text_len"]].decode("utf-8", "replace")

    def preprocess(self, samples: np.ndarray) -> np.ndarray:
        """TranscriptionWorker::preprocess_audio on a copy of the job's buffer"""
        if not self.noise_reduction and (self.audio_config is None or not self.audio_config.preprocessing):
            return samples
        buf = E.AudioBuffer(np.array(samples, dtype=np.float32, order="C"), SAMPLE_RATE)
        buf.preprocess(self.audio_config, self.noise_reduction, self.noise_reduction_strength, self.denoiser)
        return buf.samples

    def transcribe_job(self, job: ChunkJob) -> ChunkResult:
        s_all = self.preprocess(job.samples)
        if self.vad is not None and float(self.vad(s_all)) < self.vad_threshold:
            self.skipped_silent += 1
            self.context = []
            text = ""
        else:
            # the worker hands the WHOLE buffer to engine.transcribe (worker.rs:152): a job longer than 30 s (a late timer
            # tick, a long VAD segment in continuous mode) is cut at the 30 s marks like any other input, window after window
            parts = []
            token_probs, word_probs = [], []
            n_ctx = self.audio_ctx if self.audio_ctx > 0 else (
                min(E.audio_ctx_for(len(s_all)), self.ctx.hp.n_audio_ctx) if self.audio_ctx < 0 and len(s_all) <= E.CHUNK_SAMPLES else 0)
            self.state.set_audio_ctx(n_ctx)
            for off in range(0, len(s_all), E.CHUNK_SAMPLES):
                s = s_all[off:off + E.CHUNK_SAMPLES]
                if n_ctx > 0 and len(s) > n_ctx * 320:
                    raise E.WhisperError(E.OHW_E_INVALID_ARG, f"audio_ctx {n_ctx} covers {n_ctx * 320} samples, window {off // E.CHUNK_SAMPLES} holds {len(s)}")
                self.state.mel(s[None, :], [len(s)], E.OHW_MEL_ZERO_TAIL, want=False)
                self.state.encode(1)
                if self.carry_context:
                    self.state.set_window_prompt([self.context] if self.context else None)
                if self.beam_size >= 2:
                    toks = self.state.beam_search(1, self.beam_size, self.params)[0]["tokens"]
                else:
                    toks = self.state.greedy(1, self.params)[0][0]
                if self.confidence:
                    self._score_window(toks, off // E.CHUNK_SAMPLES, sum(len(p) for p in parts), token_probs, word_probs)
                parts.append(b"".join(self.ctx.token_text(t) for t in toks if t < self.ctx.tok.eot))
                if self._command_table is not None:                      # of the job's last window
                    k = E.command_match_host(self._command_table, toks)
                    self.last_command = self._command_index[k] if k >= 0 else -1
                    self.last_list_logprob = float(self.state.command_list_logprob(1)[0])
                if self.carry_context:
                    self.context = E.prompt_clip([t for t in toks if t < self.ctx.tok.eot], self.ctx.hp.n_text_ctx)
                self.windows_decoded += 1
            text = b"".join(parts).decode("utf-8", "replace").strip()
            if self.confidence:
                return ChunkResult(text, job.sequence_id, job.chunk_id, job.is_final, len(job.samples) / SAMPLE_RATE, token_probs, word_probs)
        return ChunkResult(text, job.sequence_id, job.chunk_id, job.is_final, len(job.samples) / SAMPLE_RATE)

    def tick(self, recording: np.ndarray, current_pos: int, is_final: bool = False) -> List[ChunkResult]:
        """the daemon's chunk-timer arm and the worker in one call: schedule, transcribe, hand to the tracker, return what the
        tracker releases"""
        job = self.scheduler.tick(recording, current_pos, is_final)
        if job is None:
            return []
        self.tracker.add_result(self.transcribe_job(job))
        return self.tracker.take_ready()
