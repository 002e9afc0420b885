"""ctypes binding of libohw.so and a Python mirror of the reference's `WhisperEngine`.

The product path is the HIP library: nothing here computes; there is no CPU fallback and no import
of oracle/.  If libohw.so is missing or cannot be loaded this module raises at import of the
library handle (`lib()`), loudly.

Mirror of the reference interface (reference src/engine/whisper.rs):
    WhisperEngine.new(model_path, language, translate, use_gpu)   :129-179
    WhisperEngine.transcribe(AudioBuffer) -> TranscriptionResult  :204-310
    WhisperEngine.benchmark(safety_margin) -> BenchmarkResult     :334-387
    WhisperError variants                                          :14-27
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import os
import time
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OHW_LIB") or os.path.join(_HERE, "libohw.so")   # OHW_LIB: instrumented builds for tools/

CHUNK_SAMPLES = 480000
CHUNK_FRAMES = 3000

OHW_DTYPE_AUTO, OHW_DTYPE_BF16, OHW_DTYPE_F16 = -1, 0, 1
OHW_MEL_REFLECT, OHW_MEL_ZERO_TAIL = 0, 1
OHW_WINDOW_FIXED, OHW_WINDOW_SEEK, OHW_WINDOW_FIXED_RECORDING_MEL = 0, 1, 2
OHW_SCHEDULE_SEQUENTIAL, OHW_SCHEDULE_PIPELINE, OHW_SCHEDULE_LANES = 0, 1, 2
EPI_BIAS_T, EPI_BIAS_GELU_T, EPI_BIAS_RESID_F32, EPI_F32 = 0, 1, 2, 4
# which kernel ohw_dbg_cross_attn / ohw_dbg_self_attn launched (OHW_XA_* / OHW_SA_*, kernels.hpp's XattnVariant / SelfAttnVariant)
XA_PLAIN, XA_SPLIT, XA_ROWS2, XA_ROWS3, XA_ROWS4, XA_GROUP2, XA_GROUP3, XA_GROUP4, XA_GROUP5, XA_GROUP_SPLIT = range(10)
SA_PLAIN, SA_SLOTS = 0, 1

OHW_E_MODEL_NOT_FOUND, OHW_E_LOAD_FAILED, OHW_E_TRANSCRIBE = -3001, -3002, -3003
OHW_E_NO_GPU, OHW_E_OOM, OHW_E_INVALID_ARG, OHW_E_VALIDATION = -3004, -3005, -3006, -3007


class HParams(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_vocab", "n_audio_ctx", "n_audio_state", "n_audio_head", "n_audio_layer",
                                         "n_text_ctx", "n_text_state", "n_text_head", "n_text_layer", "n_mels", "ftype")]

    def as_list(self):
        return [int(getattr(self, n)) for n, _ in self._fields_]


class SpecialTokens(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("eot", "sot", "translate", "transcribe", "solm", "prev", "nosp", "no_timestamps",
                                         "timestamp_begin", "blank", "n_langs")]


class AudioInfo(C.Structure):
    _fields_ = [("error", C.c_int32), ("duration_secs", C.c_float), ("sample_count", C.c_int64), ("min_value", C.c_float),
                ("max_value", C.c_float), ("rms", C.c_float), ("nan_count", C.c_int64), ("inf_count", C.c_int64)]


class SampleParams(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("lang_id", "translate", "no_timestamps", "suppress_blank", "max_initial_ts", "n_max", "force_len")]


class PreprocessConfig(C.Structure):
    """ohw_preprocess_config: the reference's [audio] preprocessing settings (src/config.rs:1020-1070, defaults :1129-1160)"""
    _fields_ = [("preprocessing", C.c_int32), ("normalization_enabled", C.c_int32), ("normalization_target_db", C.c_float),
                ("compression_enabled", C.c_int32), ("compression_threshold_db", C.c_float), ("compression_ratio", C.c_float),
                ("compression_attack_ms", C.c_float), ("compression_release_ms", C.c_float), ("compression_makeup_gain_db", C.c_float),
                ("limiter_enabled", C.c_int32), ("limiter_ceiling_db", C.c_float), ("limiter_release_ms", C.c_float)]


class GreedyResult(C.Structure):
    _fields_ = [("tokens", C.POINTER(C.c_int32)), ("n_tokens", C.POINTER(C.c_int32)), ("sum_logprob", C.POINTER(C.c_float)),
                ("token_logprobs", C.POINTER(C.c_float)), ("ended_by_eot", C.POINTER(C.c_int32)), ("no_speech_prob", C.POINTER(C.c_float))]


class VadConfig(C.Structure):
    """reference src/vad/mod.rs:57-100"""
    _fields_ = [("enabled", C.c_int32), ("threshold", C.c_float), ("min_silence_ms", C.c_uint32), ("min_speech_ms", C.c_uint32),
                ("speech_pad_ms", C.c_uint32)]


class SpeechSegment(C.Structure):
    _fields_ = [("start", C.c_int64), ("end", C.c_int64), ("avg_probability", C.c_float)]


class VadDetector(C.Structure):
    """ohw_vad_detector: the device detector's noise-floor quantile, margin and slope (defaults 0.10, 9 dB, 3 dB)"""
    _fields_ = [("floor_quantile", C.c_float), ("margin_db", C.c_float), ("slope_db", C.c_float)]


class ChunkPlan(C.Structure):
    """ohw_chunk_plan (defaults 30 s, 2000 ms, 1100 ms)"""
    _fields_ = [("max_chunk_s", C.c_float), ("max_gap_ms", C.c_uint32), ("min_chunk_ms", C.c_uint32)]


class SpeechChunk(C.Structure):
    _fields_ = [("start", C.c_int64), ("end", C.c_int64), ("first_segment", C.c_int32), ("n_segments", C.c_int32)]


class FrameProbs(C.Structure):
    _fields_ = [("p", C.POINTER(C.c_float)), ("n", C.c_int64), ("frame_samples", C.c_int32)]


DENOISE_FRAME_FN = C.CFUNCTYPE(C.c_float, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float))
DENOISE_RESET_FN = C.CFUNCTYPE(None, C.c_void_p)


class DenoiseEngineC(C.Structure):
    """ohw_denoise_engine: where a host plugs in nnnoiseless::DenoiseState (reference src/input/audio.rs:275-293)"""
    _fields_ = [("user", C.c_void_p), ("process_frame", DENOISE_FRAME_FN), ("reset", DENOISE_RESET_FN)]


VAD_PROCESS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_float), C.c_int64, C.POINTER(C.c_float))
VAD_RESET_FN = C.CFUNCTYPE(None, C.c_void_p)


class VadEngineC(C.Structure):
    _fields_ = [("user", C.c_void_p), ("process", VAD_PROCESS_FN), ("reset", VAD_RESET_FN), ("chunk_size", C.c_int32), ("sample_rate", C.c_uint32)]


class BeamResult(C.Structure):
    _fields_ = [("tokens", C.POINTER(C.c_int32)), ("n_tokens", C.POINTER(C.c_int32)), ("sum_logprob", C.POINTER(C.c_float)),
                ("n_finished", C.POINTER(C.c_int32))]


class DbgBeamIO(C.Structure):
    """ohw_dbg_beam_io"""
    _fields_ = ([(n, C.c_int32) for n in ("first", "K", "W", "side")] + [("logits", C.POINTER(C.c_float))] +
                [(n, C.POINTER(C.c_float) if n in ("beam_sum", "fin_sum", "cand_lp") else C.POINTER(C.c_int32))
                 for n in ("tokens", "kv_slot", "n_cur", "n_past_w", "win_done", "beam_sum", "fin_cnt", "fin_tok", "fin_len", "fin_sum",
                           "cand_tok", "cand_lp", "tokens_next", "kv_slot_next", "next_tok", "n_past", "n_done")] +
                [("tickets_out", C.POINTER(C.c_uint32))])


class DbgSampleIO(C.Structure):
    """ohw_dbg_sample_io"""
    _fields_ = ([("batch", C.c_int32), ("advance", C.c_int32), ("temperature", C.c_float), ("logits", C.POINTER(C.c_float)),
                 ("uniforms", C.POINTER(C.c_double))] +
                [(n, C.POINTER(C.c_float) if n in ("sum_logprob", "tok_lp", "nosp_prob") else C.POINTER(C.c_int32))
                 for n in ("tokens", "n_cur", "n_past", "done", "sum_logprob", "next_tok", "tok_lp", "nosp_prob", "n_done")] +
                [("tickets_out", C.POINTER(C.c_uint32))])


class BeamResultEx(C.Structure):
    """ohw_beam_result_ex"""
    _fields_ = [("tokens", C.POINTER(C.c_int32)), ("n_tokens", C.POINTER(C.c_int32)), ("sum_logprob", C.POINTER(C.c_float)),
                ("n_finished", C.POINTER(C.c_int32)), ("token_logprobs", C.POINTER(C.c_float)), ("ended_by_eot", C.POINTER(C.c_int32)),
                ("no_speech_prob", C.POINTER(C.c_float))]


class DbgBeamIOEx(C.Structure):
    """ohw_dbg_beam_io_ex"""
    _fields_ = [("base", DbgBeamIO), ("plog", C.POINTER(C.c_float)), ("plog_next", C.POINTER(C.c_float)), ("fin_plog", C.POINTER(C.c_float)),
                ("nosp_prob", C.POINTER(C.c_float))]


class BeamFinishIO(C.Structure):
    """ohw_beam_finish_io"""
    _fields_ = ([(n, C.c_int32) for n in ("K", "W", "stride", "max_tokens")] +
                [(n, C.POINTER(C.c_float) if n in ("fin_sum", "fin_plog", "plog", "beam_sum", "out_logprobs", "sum_logprob") else C.POINTER(C.c_int32))
                 for n in ("fin_cnt", "fin_len", "fin_sum", "fin_tok", "fin_plog", "n_cur", "tokens", "plog", "beam_sum", "out_tokens",
                           "out_logprobs", "n_tokens", "sum_logprob", "ended_by_eot", "n_finished")])


class DbgDecGemmIO(C.Structure):
    """ohw_dbg_dec_gemm_io: every pointer but n_past and shape_out is a device address"""
    _fields_ = ([(n, C.c_int32) for n in ("dtype", "epilogue", "form", "M", "N", "K", "n_new")] + [("ld_out", C.c_int64)] +
                [(n, C.c_int32) for n in ("cu_budget", "ksplit")] +
                [(n, C.c_void_p) for n in ("w", "bias", "gamma", "beta", "x", "stat_in", "out", "slab")] + [("slab_bytes", C.c_int64)] +
                [(n, C.c_void_p) for n in ("ticket", "x16_out", "stat_out", "k_cache", "v_cache")] + [("n_past", C.POINTER(C.c_int32))] +
                [(n, C.c_int32) for n in ("d_model", "n_head", "n_ctx")] + [("shape_out", C.POINTER(C.c_int32))])


class DbgLogitsRowsIO(C.Structure):
    """ohw_dbg_logits_rows_io: ohw_dbg_dec_gemm_io with epilogue LOGITS, plus the all-rows output (a device address, or None)"""
    _fields_ = [("g", DbgDecGemmIO), ("out_all", C.c_void_p), ("ld_all", C.c_int64)]


class TokenScore(C.Structure):
    """ohw_token_score: the five words of one raw logits row (include/ohw.h, "confidence")"""
    _fields_ = [("logit", C.c_float), ("lse_text", C.c_float), ("lse_all", C.c_float), ("top_id", C.c_int32), ("top_logit", C.c_float)]


# numpy's view of ohw_token_score (20 bytes, no padding)
TOKEN_SCORE_DTYPE = np.dtype([("logit", np.float32), ("lse_text", np.float32), ("lse_all", np.float32), ("top_id", np.int32), ("top_logit", np.float32)])
assert TOKEN_SCORE_DTYPE.itemsize == C.sizeof(TokenScore) == 20


class DbgEncGemmIO(C.Structure):
    """ohw_dbg_enc_gemm_io: a, w, bias, pos and out are device addresses, c_row_map is a host table"""
    _fields_ = ([(n, C.c_int32) for n in ("dtype", "epilogue", "kernel", "conv_cin")] +
                [(n, C.c_int64) for n in ("M", "N", "K", "lda", "a_batch_stride", "rows_per_batch", "ldc", "c_batch_stride")] +
                [(n, C.c_int32) for n in ("d_model", "n_head", "t_len", "batch", "batch_offset")] + [("c_row_map", C.POINTER(C.c_int32))] +
                [("a", C.c_void_p), ("a_elems", C.c_int64), ("w", C.c_void_p), ("bias", C.c_void_p), ("pos", C.c_void_p), ("out", C.c_void_p),
                 ("out_elems", C.c_int64)])


# ohw_dbg_enc_gemm: every epilogue of gemm.hpp's GemmEpilogue and the kernel to run (OHW_EG_KERNEL_*)
EPI_GELU_POS_F32, EPI_CROSSKV_T = 3, 5
EG_KERNEL_AUTO, EG_KERNEL_K128, EG_KERNEL_SMALL, EG_KERNEL_K256 = range(4)

# ohw_dbg_dec_gemm: epilogues (kernels.hpp's DecEpilogue), operand forms and the work shape that ran (DecGemmShape)
DEPI_QKV, DEPI_BIAS_T, DEPI_BIAS_GELU_T, DEPI_BIAS_RESID, DEPI_LOGITS = range(5)
DG_FORM_PLAIN, DG_FORM_LN, DG_FORM_PN = range(3)
DG_SHAPE_1x1, DG_SHAPE_2x1, DG_SHAPE_1x2, DG_SHAPE_2x2, DG_SHAPE_4x2, DG_SHAPE_1x6, DG_SHAPE_4x6, DG_SHAPE_5x6 = range(8)

OHW_DBG_SENTINEL_I32 = -7777777
OHW_DBG_SENTINEL_F32 = -12345.0


def _beam_finish(handle, K: int, state: dict, max_tokens: Optional[int]) -> dict:
    W = int(np.asarray(state["n_cur"]).size)
    R = W * K
    S = int(np.asarray(state["tokens"]).shape[1])
    n = S if max_tokens is None else int(max_tokens)
    i32 = lambda k, shape: np.array(state[k], dtype=np.int32, order="C").reshape(shape)
    f32 = lambda k, shape: np.array(state[k], dtype=np.float32, order="C").reshape(shape)
    a = dict(fin_cnt=i32("fin_cnt", W), fin_len=i32("fin_len", R), fin_sum=f32("fin_sum", R), fin_tok=i32("fin_tok", (R, S)),
             fin_plog=f32("fin_plog", (R, S + 1)), n_cur=i32("n_cur", W), tokens=i32("tokens", (R, S)), plog=f32("plog", (R, S + 1)),
             beam_sum=f32("beam_sum", R), out_tokens=np.zeros((W, max(n, 0)), np.int32), out_logprobs=np.zeros((W, max(n, 0) + 1), np.float32),
             n_tokens=np.zeros(W, np.int32), sum_logprob=np.zeros(W, np.float32), ended_by_eot=np.zeros(W, np.int32),
             n_finished=np.zeros(W, np.int32))
    io = BeamFinishIO(K, W, S, n, *[(_fp(a[k]) if a[k].dtype == np.float32 else _ip(a[k])) for k, _ in BeamFinishIO._fields_[4:]])
    _check(lib().ohw_beam_finish_host(C.byref(io)) if handle is None else lib().ohw_dbg_beam_finish(handle, C.byref(io)))
    return {"tokens": a["out_tokens"], "logprobs": a["out_logprobs"], "n_tokens": a["n_tokens"], "sum_logprob": a["sum_logprob"],
            "ended_by_eot": a["ended_by_eot"], "n_finished": a["n_finished"]}


def beam_finish_host(K: int, state: dict, max_tokens: Optional[int] = None) -> dict:
    """ohw_beam_finish_host: the final ranking of a beam search on the host, no GPU.  state: fin_cnt / n_cur [W], fin_len /
    fin_sum / beam_sum [R], fin_tok / tokens [R][S], fin_plog / plog [R][S + 1] (R = W * K; S: any row length).
    -> dict(tokens [W][max_tokens], logprobs [W][max_tokens + 1], n_tokens, sum_logprob, ended_by_eot, n_finished [W]); what the
    rule did not write holds OHW_DBG_SENTINEL_*"""
    return _beam_finish(None, K, state, max_tokens)


PHRASE_MAX_LEN, PHRASE_MAX_PHRASES = 16, 1024
PHRASE_MAX_NODES = 1 + PHRASE_MAX_PHRASES * (PHRASE_MAX_LEN - 1)
PHRASE_MAX_EDGES = PHRASE_MAX_PHRASES * PHRASE_MAX_LEN
PHRASE_MAX_PATH = PHRASE_MAX_PHRASES * (PHRASE_MAX_LEN - 1) * PHRASE_MAX_LEN // 2


class PhraseTableC(C.Structure):
    _fields_ = [("n_phrases", C.c_int32), ("n_nodes", C.c_int32), ("n_edges", C.c_int32), ("n_path", C.c_int32),
                ("depth_start", C.c_int32 * (PHRASE_MAX_LEN + 1)), ("path_base", C.c_int32 * PHRASE_MAX_LEN),
                ("child_off", C.POINTER(C.c_int32)), ("path", C.POINTER(C.c_int32)), ("child_tok", C.POINTER(C.c_int32)),
                ("child_boost", C.POINTER(C.c_float))]


class PhraseTable:
    """ohw_phrase_table with the arrays it points into: the flat trie of a hot-phrase table (include/ohw.h states the layout)"""

    def __init__(self):
        self.child_off = np.zeros(PHRASE_MAX_NODES + 1, dtype=np.int32)
        self.path = np.zeros(PHRASE_MAX_PATH, dtype=np.int32)
        self.child_tok = np.zeros(PHRASE_MAX_EDGES, dtype=np.int32)
        self.child_boost = np.zeros(PHRASE_MAX_EDGES, dtype=np.float32)
        self.c = PhraseTableC()
        self.c.child_off, self.c.path, self.c.child_tok, self.c.child_boost = _ip(self.child_off), _ip(self.path), _ip(self.child_tok), _fp(self.child_boost)

    def arrays(self) -> dict:
        """the table's used parts, copied: depth_start [17], path_base [16], child_off [n_nodes + 1], path, child_tok, child_boost"""
        c = self.c
        return {"n_phrases": int(c.n_phrases), "depth_start": np.array(c.depth_start[:], dtype=np.int32), "path_base": np.array(c.path_base[:], dtype=np.int32),
                "child_off": self.child_off[:c.n_nodes + 1].copy(), "path": self.path[:c.n_path].copy(),
                "child_tok": self.child_tok[:c.n_edges].copy(), "child_boost": self.child_boost[:c.n_edges].copy()}

    def boost_host(self, history: Sequence[int], n_cur: int, row: np.ndarray) -> np.ndarray:
        """ohw_phrase_boost_host: the rule on a copy of one row [n_vocab], history = the row's own sampled tokens"""
        out = np.ascontiguousarray(row, dtype=np.float32).copy()
        h = np.ascontiguousarray(list(history) or [0], dtype=np.int32)
        _check(lib().ohw_phrase_boost_host(C.byref(self.c), _ip(h), int(n_cur), _fp(out), int(out.size)))
        return out


def _dbg_rule_rows(logits, histories, n_cur, done, group):
    """what the three rule test entries take: a copy of logits [rows][ld] (it comes back changed), histories [entries * group][max_tokens],
    n_cur (None stays None) and done [entries]"""
    lg = np.ascontiguousarray(logits, dtype=np.float32).copy()
    h = np.ascontiguousarray(histories, dtype=np.int32)
    dn = np.ascontiguousarray(done, dtype=np.int32)
    nc = None if n_cur is None else np.ascontiguousarray(n_cur, dtype=np.int32)
    assert lg.ndim == 2 and h.ndim == 2 and h.shape[0] == dn.size * group and (nc is None or nc.size == dn.size)
    return lg, h, nc, dn


def _flat_phrases(phrases, boosts):
    """token lists -> (tokens, offsets, boosts) as the C ABI takes them"""
    lens = [len(p) for p in phrases]
    off = np.zeros(len(lens) + 1, dtype=np.int32)
    off[1:] = np.cumsum(lens, dtype=np.int64)
    toks = np.ascontiguousarray([t for p in phrases for t in p] or [0], dtype=np.int32)
    b = np.ascontiguousarray(list(boosts) or [0.0], dtype=np.float32)
    if len(boosts) != len(lens):
        raise ValueError("one boost per phrase")
    return toks, off, b


def phrase_table_build_host(phrases: Sequence[Sequence[int]], boosts: Sequence[float], eot: int) -> PhraseTable:
    """ohw_phrase_table_build_host: token-id phrases with a boost each -> the flat trie; needs no device"""
    toks, off, b = _flat_phrases(phrases, boosts)
    t = PhraseTable()
    _check(lib().ohw_phrase_table_build_host(_ip(toks), _ip(off), _fp(b), len(phrases), int(eot), C.byref(t.c)))
    return t


def parse_hot_phrases(text: str, default_boost: float) -> Tuple[List[str], List[float]]:
    """a hot-phrase file: one phrase per line, optionally a tab and its boost; empty lines and lines starting with # are skipped"""
    phrases, boosts = [], []
    for ln, line in enumerate(text.splitlines(), 1):
        line = line.strip("\r\n")
        if not line.strip() or line.lstrip().startswith("#"):
            continue
        phrase, tab, boost = line.partition("\t")
        try:
            b = float(boost) if tab and boost.strip() else float(default_boost)
        except ValueError:
            raise ValueError(f"hot phrases, line {ln}: the boost {boost!r} is not a number") from None
        if not phrase.strip():
            raise ValueError(f"hot phrases, line {ln}: no phrase in front of the tab")
        phrases.append(phrase.strip())
        boosts.append(b)
    return phrases, boosts


def _hot_phrase_args(phrases, boost):
    """(strings or token lists, a boost or one per phrase) -> (is_text, phrases, boosts)"""
    phrases = list(phrases or [])
    boosts = [float(boost)] * len(phrases) if np.isscalar(boost) else [float(b) for b in boost]
    if len(boosts) != len(phrases):
        raise ValueError("hot phrases: one boost per phrase, or one for all")
    is_text = [isinstance(p, (str, bytes)) for p in phrases]
    if any(is_text) and not all(is_text):
        raise ValueError("hot phrases: strings or token lists, not both in one call")
    return bool(phrases) and is_text[0], phrases, boosts


def hot_phrase_tokens(ctx, phrases, boost=1.0) -> Tuple[List[List[int]], List[float]]:
    """what ohw_engine_set_hot_phrases does with its texts, for a caller that owns a State: every string in two variants, with a
    leading space and as given, duplicates dropped; token lists pass through -> (token lists, boosts)"""
    is_text, phrases, boosts = _hot_phrase_args(phrases, boost)
    if not is_text:
        return [list(p) for p in phrases], boosts
    out, bs = [], []
    for i, (p, b) in enumerate(zip(phrases, boosts)):
        raw = _text_bytes(p)
        forms = [t for t in (ctx.tokenize(b" " + raw), ctx.tokenize(raw)) if t]      # a form with no token in the vocabulary is dropped
        if not forms:
            raise ValueError(f"hot phrases: text {i} has no token in this vocabulary")
        for t in forms:
            if t not in out:
                out.append(t)
                bs.append(b)
    return out, bs


REPEAT_BAN = np.float32(-1.0e30)         # OHW_REPEAT_BAN
REPEAT_PENALTY_MIN, REPEAT_PENALTY_MAX, REPEAT_MAX_NGRAM = 0.01, 100.0, 32


def repeat_rule_host(penalty: float, ngram: int, history: Sequence[int], n_cur: int, row: np.ndarray, eot: int) -> np.ndarray:
    """ohw_repeat_rule_host: repetition penalty and no-repeat n-grams on a copy of one row [n_vocab]; history = the row's own
    sampled tokens (include/ohw.h states the rule); needs no device"""
    out = np.ascontiguousarray(row, dtype=np.float32).copy()
    h = np.ascontiguousarray(list(history) or [0], dtype=np.int32)
    _check(lib().ohw_repeat_rule_host(float(penalty), int(ngram), _ip(h), int(n_cur), _fp(out), int(out.size), int(eot)))
    return out


COMMAND_PENALTY_MAX, COMMAND_PENALTY_DEFAULT = 1000.0, 100.0
COMMAND_MAX_NODES = 1 + PHRASE_MAX_PHRASES * PHRASE_MAX_LEN
COMMAND_MAX_EDGES = PHRASE_MAX_PHRASES * PHRASE_MAX_LEN
COMMAND_MAX_PATH = PHRASE_MAX_PHRASES * PHRASE_MAX_LEN * (PHRASE_MAX_LEN + 1) // 2


class CommandTableC(C.Structure):
    _fields_ = [("n_phrases", C.c_int32), ("n_nodes", C.c_int32), ("n_edges", C.c_int32), ("n_path", C.c_int32), ("eot", C.c_int32),
                ("depth_start", C.c_int32 * (PHRASE_MAX_LEN + 2)), ("path_base", C.c_int32 * (PHRASE_MAX_LEN + 1)),
                ("child_off", C.POINTER(C.c_int32)), ("path", C.POINTER(C.c_int32)), ("child_tok", C.POINTER(C.c_int32)),
                ("terminal", C.POINTER(C.c_int32)), ("phrase_id", C.POINTER(C.c_int32))]


class CommandHit(C.Structure):
    _fields_ = [("window", C.c_int32), ("phrase", C.c_int32), ("list_logprob", C.c_float)]


class CommandTable:
    """ohw_command_table with the arrays it points into: the anchored flat trie of a command list (include/ohw.h states the layout)"""

    def __init__(self):
        self.child_off = np.zeros(COMMAND_MAX_NODES + 1, dtype=np.int32)
        self.path = np.zeros(COMMAND_MAX_PATH, dtype=np.int32)
        self.child_tok = np.zeros(COMMAND_MAX_EDGES, dtype=np.int32)
        self.terminal = np.zeros(COMMAND_MAX_NODES, dtype=np.int32)
        self.phrase_id = np.zeros(COMMAND_MAX_NODES, dtype=np.int32)
        self.c = CommandTableC()
        self.c.child_off, self.c.path, self.c.child_tok = _ip(self.child_off), _ip(self.path), _ip(self.child_tok)
        self.c.terminal, self.c.phrase_id = _ip(self.terminal), _ip(self.phrase_id)

    def arrays(self) -> dict:
        """the table's used parts, copied: depth_start [18], path_base [17], child_off [n_nodes + 1], path, child_tok, terminal, phrase_id"""
        c = self.c
        return {"n_phrases": int(c.n_phrases), "eot": int(c.eot), "depth_start": np.array(c.depth_start[:], dtype=np.int32),
                "path_base": np.array(c.path_base[:], dtype=np.int32), "child_off": self.child_off[:c.n_nodes + 1].copy(),
                "path": self.path[:c.n_path].copy(), "child_tok": self.child_tok[:c.n_edges].copy(),
                "terminal": self.terminal[:c.n_nodes].copy(), "phrase_id": self.phrase_id[:c.n_nodes].copy()}


def command_table_build_host(phrases: Sequence[Sequence[int]], eot: int) -> CommandTable:
    """ohw_command_table_build_host: token-id phrases -> the anchored trie; needs no device"""
    toks, off, _ = _flat_phrases(phrases, [0.0] * len(phrases))
    t = CommandTable()
    _check(lib().ohw_command_table_build_host(_ip(toks), _ip(off), len(phrases), int(eot), C.byref(t.c)))
    return t


def command_rule_host(table: CommandTable, penalty: float, history: Sequence[int], n_cur: int, row: np.ndarray, eot: int) -> Tuple[np.ndarray, Optional[float]]:
    """ohw_command_rule_host: the command-list rule on a copy of one row [n_vocab]; history = the row's own sampled tokens
    (include/ohw.h states the rule); needs no device -> (the row, list_logprob or None when the history holds a text token)"""
    out = np.ascontiguousarray(row, dtype=np.float32).copy()
    h = np.ascontiguousarray(list(history) or [0], dtype=np.int32)
    lp = C.c_float(float("nan"))
    has_text = any(0 <= int(t) < int(eot) for t in list(history)[:int(n_cur)])
    _check(lib().ohw_command_rule_host(C.byref(table.c), float(penalty), _ip(h), int(n_cur), _fp(out), int(out.size), int(eot), C.byref(lp)))
    return out, (None if has_text else float(lp.value))


def command_match_host(table: CommandTable, tokens: Sequence[int]) -> int:
    """ohw_command_match_host: the index of the listed phrase that the text tokens of `tokens` equal exactly (the lowest, among
    duplicates), else -1"""
    toks = list(tokens)
    t = np.ascontiguousarray(toks or [0], dtype=np.int32)
    return int(lib().ohw_command_match_host(C.byref(table.c), _ip(t), len(toks)))


def parse_commands(text: str) -> List[str]:
    """a command file: one phrase per line; empty lines and lines starting with # are skipped"""
    return [line.strip() for line in text.splitlines() if line.strip() and not line.lstrip().startswith("#")]


def command_penalty_arg(v) -> float:
    """a command penalty as the C ABI accepts it: 0 < p <= 1000, or inf; ValueError otherwise"""
    try:
        x = float(v)
    except (TypeError, ValueError):
        x = float("nan")
    if not (0.0 < x <= COMMAND_PENALTY_MAX or x == float("inf")):      # false for NaN
        raise ValueError(f"the command penalty must lie in (0, 1000] or be inf, not {v!r}")
    return x


def _commands_are_text(phrases) -> bool:
    is_text = [isinstance(p, (str, bytes)) for p in phrases]
    if any(is_text) and not all(is_text):
        raise ValueError("commands: strings or token lists, not both in one call")
    return bool(phrases) and is_text[0]


def command_tokens(ctx, phrases) -> Tuple[List[List[int]], List[int]]:
    """what ohw_engine_set_commands does with its texts, for a caller that owns a State: every string as given and with a leading
    space, a form without a token or equal to the other dropped; token lists pass through -> (token lists, the caller's index of each)"""
    phrases = list(phrases or [])
    if not _commands_are_text(phrases):
        return [list(p) for p in phrases], list(range(len(phrases)))
    out, index = [], []
    for i, p in enumerate(phrases):
        raw = _text_bytes(p)
        forms = [t for t in (ctx.tokenize(raw), ctx.tokenize(b" " + raw)) if t]
        if not forms:
            raise ValueError(f"commands: text {i} has no token in this vocabulary")
        for k, t in enumerate(forms):
            if k == 0 or t != forms[0]:
                out.append(t)
                index.append(i)
    return out, index


def _commands_text_call(fn, handle, phrases, penalty):
    raw = [_text_bytes(p) for p in phrases]
    arr = (C.c_char_p * max(len(raw), 1))(*raw)
    _check(fn(handle, arr, len(raw), float(penalty)))


def _hot_phrase_text_call(fn, handle, phrases, boosts):
    raw = [_text_bytes(p) for p in phrases]
    arr = (C.c_char_p * max(len(raw), 1))(*raw)
    b = np.ascontiguousarray(boosts or [0.0], dtype=np.float32)
    _check(fn(handle, arr, _fp(b), len(raw)))


class WindowQuality(C.Structure):
    _fields_ = [("n_tokens", C.c_int32), ("avg_logprob", C.c_float), ("entropy", C.c_float), ("would_fallback", C.c_int32),
                ("temperature", C.c_float), ("no_speech_prob", C.c_float), ("no_speech", C.c_int32), ("seek_delta", C.c_int32),
                ("result_len", C.c_int32), ("failed", C.c_int32)]


class DecodePolicy(C.Structure):
    """ohw_decode_policy: whisper.cpp's defaults (temperature_inc 0.2, entropy_thold 2.4, logprob_thold -1.0, no_speech_thold 0.6)"""
    _fields_ = [("temperature_inc", C.c_float), ("entropy_thold", C.c_float), ("logprob_thold", C.c_float), ("no_speech_thold", C.c_float)]


class SeqEval(C.Structure):
    """ohw_seq_eval: one sampled sequence as whisper.cpp's loop bookkeeping judges it"""
    _fields_ = [("n_sampled", C.c_int32), ("result_len", C.c_int32), ("n_keep", C.c_int32), ("seek_delta", C.c_int32),
                ("failed", C.c_int32), ("completed", C.c_int32), ("avg_logprob", C.c_float), ("entropy", C.c_float)]


class AudioSpan(C.Structure):
    _fields_ = [("samples", C.POINTER(C.c_float)), ("n", C.c_int64)]


class AlignHead(C.Structure):
    _fields_ = [("layer", C.c_int32), ("head", C.c_int32)]


class TokenTime(C.Structure):
    _fields_ = [("id", C.c_int32), ("window", C.c_int32), ("t0", C.c_float), ("t1", C.c_float)]


class TokenProb(C.Structure):
    """ohw_token_prob"""
    _fields_ = [("id", C.c_int32), ("window", C.c_int32), ("logprob_text", C.c_float), ("logprob_all", C.c_float), ("logprob_decode", C.c_float),
                ("top_id", C.c_int32), ("top_logprob_text", C.c_float)]


class WordProb(C.Structure):
    """ohw_word_prob"""
    _fields_ = [("text_off", C.c_size_t), ("text_len", C.c_size_t), ("probability", C.c_float)]


class SegmentInfo(C.Structure):
    """ohw_segment_info"""
    _fields_ = [("avg_logprob_text", C.c_float), ("no_speech_prob", C.c_float), ("temperature", C.c_float)]


class ScoreResultC(C.Structure):
    """ohw_score_result"""
    _fields_ = [("tokens", C.POINTER(TokenProb)), ("n_tokens", C.c_int32), ("eot", TokenProb), ("sum_logprob_all", C.c_float)]


class SpanTime(C.Structure):
    _fields_ = [("text_off", C.c_size_t), ("text_len", C.c_size_t), ("t0", C.c_float), ("t1", C.c_float)]


class TokenSpan(C.Structure):
    _fields_ = [("first", C.c_int32), ("end", C.c_int32), ("t0", C.c_float), ("t1", C.c_float)]


class Timings(C.Structure):
    _fields_ = [("mel_ms", C.c_float), ("encode_ms", C.c_float), ("decode_ms", C.c_float), ("total_ms", C.c_float), ("decode_steps", C.c_int32)]


AUDIO_ERRORS = {0: "Ok", 1: "Empty", 2: "InvalidSampleRate", 3: "TooLong", 4: "TooShort", 5: "ContainsNaN", 6: "ContainsInfinite"}

# every symbol include/ohw.h declares
EXPORTS = [
    "ohw_validate_audio", "ohw_ctx_create", "ohw_ctx_create_synthetic", "ohw_ctx_info", "ohw_token_text", "ohw_ctx_free",
    "ohw_state_create", "ohw_state_free", "ohw_state_set_stream", "ohw_state_max_batch", "ohw_mel", "ohw_recording_set", "ohw_mel_seek", "ohw_encode", "ohw_decode",
    "ohw_default_sample_params", "ohw_sample_greedy_host", "ohw_greedy", "ohw_state_timings", "ohw_engine_new",
    "ohw_engine_transcribe", "ohw_engine_last_tokens", "ohw_engine_benchmark", "ohw_engine_free", "ohw_engine_state",
    "ohw_engine_ctx", "ohw_lang_id_to_code", "ohw_lang_code_to_id", "ohw_last_error", "ohw_abi_version", "ohw_state_fetch",
    "ohw_dbg_gemm", "ohw_dbg_attention", "ohw_state_profile_begin", "ohw_state_profile_end", "ohw_ctx_weight_digest", "ohw_detect_language", "ohw_state_ctx", "ohw_engine_set_window_mode", "ohw_engine_last_text", "ohw_engine_last_quality",
    "ohw_stream_create", "ohw_stream_destroy", "ohw_stream_wait", "ohw_stream_sync",
    "ohw_ctx_create_shell", "ohw_ctx_blob_size", "ohw_ctx_blob_export", "ohw_ctx_blob_import",
    "ohw_default_preprocess_config", "ohw_preprocess_audio", "ohw_dsp_rms_db", "ohw_dsp_apply_gain", "ohw_dsp_normalize_rms",
    "ohw_dsp_compress", "ohw_dsp_limit", "ohw_dsp_resample_linear",
    "ohw_tracker_new", "ohw_tracker_free", "ohw_tracker_add_pending", "ohw_tracker_add_result", "ohw_tracker_take_ready", "ohw_tracker_ready_get",
    "ohw_tracker_reset_dedup", "ohw_tracker_is_empty", "ohw_tracker_is_pending", "ohw_tracker_pending_count", "ohw_tracker_waiting_count", "ohw_extract_chunk",
    "ohw_chunk_scheduler_new", "ohw_chunk_scheduler_free", "ohw_chunk_scheduler_tick", "ohw_chunk_scheduler_position", "ohw_chunk_scheduler_next_id",
    "ohw_chunk_scheduler_rejected", "ohw_resampler_create", "ohw_resampler_free", "ohw_resampler_out_len", "ohw_resampler_run", "ohw_greedy_ex", "ohw_state_set_logit_bias", "ohw_state_set_batch_invariant", "ohw_dbg_sample",
    "ohw_decode_active", "ohw_rng_new", "ohw_rng_free", "ohw_sample_host", "ohw_default_decode_policy", "ohw_engine_set_decode_policy",
    "ohw_engine_last_trace", "ohw_engine_set_schedule", "ohw_ctx_dtype",
    "ohw_beam_search", "ohw_encode_slice", "ohw_dsp_resample_sinc", "ohw_default_vad_config", "ohw_vad_state_new", "ohw_vad_state_free", "ohw_vad_state_update",
    "ohw_vad_state_is_speech", "ohw_vad_state_speech_start", "ohw_vad_state_reset", "ohw_vad_energy_engine", "ohw_vad_energy_engine_free",
    "ohw_vad_run",
    "ohw_pool_create", "ohw_pool_transcribe", "ohw_pool_last_text", "ohw_pool_last_tokens", "ohw_pool_last_quality",
    "ohw_dbg_counter", "ohw_dsp_denoise", "ohw_denoise_passthrough_engine", "ohw_preprocess_audio_ex", "ohw_pool_set_window_mode",
    "ohw_state_set_persistent", "ohw_pool_broadcast_note", "ohw_pool_create_synthetic", "ohw_pool_set_force_len", "ohw_pool_set_schedule", "ohw_engine_set_force_len",
    "ohw_pool_set_decode_policy", "ohw_pool_n_devices", "ohw_pool_broadcast_kind", "ohw_pool_engine", "ohw_pool_free",
    "ohw_rng_uniforms", "ohw_rng_discard_draws", "ohw_sample_pass", "ohw_dbg_sample_t", "ohw_engine_set_fallback_device",
    "ohw_pool_set_fallback_device", "ohw_dequantize_host", "ohw_dbg_dequantize",
    "ohw_state_set_audio_ctx", "ohw_state_audio_ctx", "ohw_audio_ctx_for", "ohw_engine_set_audio_ctx", "ohw_pool_set_audio_ctx", "ohw_dbg_gemm_small",
    "ohw_state_set_window_ctx", "ohw_state_window_ctx", "ohw_engine_transcribe_batch", "ohw_engine_batch_result", "ohw_batch_plan",
    "ohw_state_set_packed_encoder", "ohw_state_packed_encoder", "ohw_engine_set_packed_encoder", "ohw_pool_set_packed_encoder", "ohw_dbg_poison",
    "ohw_dbg_attention_var", "ohw_dbg_cross_attn", "ohw_dbg_self_attn",
    "ohw_engine_set_detect_language", "ohw_engine_last_language", "ohw_engine_transcribe_batch_lang", "ohw_pool_set_detect_language",
    "ohw_state_set_window_lang", "ohw_state_detect_window_lang", "ohw_state_window_lang", "ohw_lang_pick_host", "ohw_dbg_lang_pick",
    "ohw_state_set_align_heads", "ohw_state_align", "ohw_align_reduce_host", "ohw_dtw_host", "ohw_dbg_align_probs", "ohw_dbg_align_reduce",
    "ohw_dbg_dtw", "ohw_engine_set_word_timestamps", "ohw_engine_last_token_times", "ohw_engine_last_words", "ohw_engine_last_segments",
    "ohw_engine_batch_times", "ohw_word_starts_host", "ohw_segments_host",
    "ohw_pool_set_word_timestamps", "ohw_pool_last_token_times", "ohw_pool_last_words", "ohw_pool_last_segments",
    "ohw_dbg_beam_step", "ohw_beam_search_ex", "ohw_dbg_beam_step_ex", "ohw_dbg_beam_finish", "ohw_beam_finish_host",
    "ohw_engine_set_beam_size", "ohw_pool_set_beam_size",
    "ohw_dbg_cross_attn_chunk",
    "ohw_state_set_window_prompt", "ohw_state_window_prompt_len", "ohw_state_prefill", "ohw_tokenize_host", "ohw_tokenize", "ohw_prompt_clip_host",
    "ohw_engine_set_initial_prompt", "ohw_engine_set_initial_prompt_tokens", "ohw_pool_set_initial_prompt",
    "ohw_recording_set_slot", "ohw_mel_seek_slots", "ohw_seek_sched_new", "ohw_seek_sched_round", "ohw_seek_sched_advance", "ohw_seek_sched_free",
    "ohw_engine_transcribe_long_batch", "ohw_engine_long_batch_quality",
    "ohw_dbg_dec_gemm", "ohw_dbg_embed", "ohw_dbg_layernorm",
    "ohw_state_set_prefill_chunk", "ohw_state_prefill_chunk", "ohw_engine_set_prefill_chunk", "ohw_dbg_cross_attn_chunk_n",
    "ohw_engine_set_carry_context", "ohw_pool_set_carry_context", "ohw_engine_last_context", "ohw_engine_long_batch_context", "ohw_carry_step_host",
    "ohw_seq_eval_host", "ohw_needs_fallback_host",
    "ohw_sample_pass_n", "ohw_dbg_sample_group", "ohw_best_of_pick_host", "ohw_engine_set_best_of", "ohw_pool_set_best_of",
    "ohw_engine_last_candidates", "ohw_engine_last_candidate_logprobs", "ohw_batch_windows_host",
    "ohw_dbg_enc_gemm",
    "ohw_phrase_table_build_host", "ohw_phrase_boost_host", "ohw_state_set_phrase_table", "ohw_state_phrase_count", "ohw_dbg_phrase_boost",
    "ohw_engine_set_hot_phrases", "ohw_engine_set_hot_phrases_tokens", "ohw_pool_set_hot_phrases",
    "ohw_repeat_rule_host", "ohw_state_set_repeat_rule", "ohw_state_repeat_rule", "ohw_dbg_repeat_rule", "ohw_engine_set_repetition",
    "ohw_pool_set_repetition",
    "ohw_command_table_build_host", "ohw_command_rule_host", "ohw_command_match_host", "ohw_state_set_command_table", "ohw_state_command_count",
    "ohw_state_command_list_logprob", "ohw_dbg_command_rule", "ohw_engine_set_commands", "ohw_engine_set_commands_tokens", "ohw_pool_set_commands",
    "ohw_engine_last_commands", "ohw_engine_batch_commands",
    "ohw_dbg_sample_ex",
    "ohw_default_vad_detector", "ohw_state_vad_frames", "ohw_speech_segments_host", "ohw_default_chunk_plan", "ohw_speech_chunks_host",
    "ohw_engine_set_vad", "ohw_engine_transcribe_speech", "ohw_engine_transcribe_speech_lang", "ohw_engine_speech_chunks",
    "ohw_engine_speech_segments", "ohw_dbg_vad_energy", "ohw_dbg_vad_floor",
    "ohw_state_score", "ohw_state_set_score_buffers", "ohw_token_score_host", "ohw_token_prob_host", "ohw_word_probs_host",
    "ohw_dbg_token_score", "ohw_dbg_logits_rows",
    "ohw_engine_set_confidence", "ohw_engine_last_token_probs", "ohw_engine_last_word_probs", "ohw_engine_last_segment_info",
    "ohw_engine_batch_confidence", "ohw_pool_set_confidence", "ohw_pool_last_token_probs", "ohw_pool_last_word_probs",
    "ohw_pool_last_segment_info", "ohw_engine_score_batch",
    "ohw_stitch_plan_host", "ohw_stitch_seams_host", "ohw_stitch_ranges_host", "ohw_stitch_clip_segment_host", "ohw_stitch_seams", "ohw_dbg_stitch",
    "ohw_engine_set_stitch", "ohw_engine_stitch", "ohw_engine_last_seams", "ohw_engine_last_window_tokens",
]


class WhisperError(RuntimeError):
    """reference src/engine/whisper.rs:14-27"""
    def __init__(self, code: int, msg: str):
        super().__init__(msg)
        self.code = code


class ModelNotFound(WhisperError):
    pass


class LoadFailed(WhisperError):
    pass


class TranscriptionFailed(WhisperError):
    pass


class ValidationFailed(WhisperError):
    def __init__(self, code: int, msg: str, info: Optional[AudioInfo] = None):
        super().__init__(code, msg)
        self.info = info
        self.kind = AUDIO_ERRORS.get(info.error, "?") if info is not None else "?"


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: build it with `python -m openhush_amd.build` (no fallback path exists)")
        L = C.CDLL(LIB_PATH)
        vp, fp, ip = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32)
        L.ohw_last_error.restype = C.c_char_p
        L.ohw_lang_id_to_code.restype = C.c_char_p
        L.ohw_lang_id_to_code.argtypes = [C.c_int32]
        L.ohw_lang_code_to_id.argtypes = [C.c_char_p]
        L.ohw_validate_audio.argtypes = [fp, C.c_int64, C.c_uint32, C.POINTER(AudioInfo)]
        L.ohw_ctx_create.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(vp)]
        L.ohw_ctx_create_synthetic.argtypes = [C.POINTER(HParams), C.c_uint32, C.c_int, C.c_int, C.POINTER(vp)]
        L.ohw_ctx_info.argtypes = [vp, C.POINTER(HParams), C.POINTER(SpecialTokens)]
        L.ohw_ctx_dtype.argtypes = [vp]
        L.ohw_ctx_create_shell.argtypes = [C.POINTER(HParams), C.c_int, C.c_int, C.POINTER(vp)]
        L.ohw_ctx_blob_size.argtypes = [vp]
        L.ohw_ctx_blob_size.restype = C.c_size_t
        L.ohw_ctx_blob_export.argtypes = [vp, vp, C.c_size_t]
        L.ohw_ctx_blob_import.argtypes = [vp, vp, C.c_size_t]
        L.ohw_token_text.argtypes = [vp, C.c_int32, C.POINTER(C.c_char_p)]
        L.ohw_ctx_free.argtypes = [vp]
        L.ohw_ctx_free.restype = None
        L.ohw_state_create.argtypes = [vp, C.c_int, C.POINTER(vp)]
        L.ohw_state_free.argtypes = [vp]
        L.ohw_state_free.restype = None
        L.ohw_state_set_stream.argtypes = [vp, vp]
        L.ohw_default_preprocess_config.argtypes = [C.POINTER(PreprocessConfig)]
        L.ohw_default_preprocess_config.restype = None
        L.ohw_preprocess_audio.argtypes = [fp, C.c_int64, C.c_uint32, C.POINTER(PreprocessConfig)]
        L.ohw_dsp_denoise.argtypes = [fp, C.c_int64, C.c_uint32, C.c_float, C.POINTER(DenoiseEngineC)]
        L.ohw_denoise_passthrough_engine.argtypes = [C.POINTER(DenoiseEngineC)]
        L.ohw_denoise_passthrough_engine.restype = None
        L.ohw_preprocess_audio_ex.argtypes = [fp, C.c_int64, C.c_uint32, C.POINTER(PreprocessConfig), C.c_int, C.c_float, C.POINTER(DenoiseEngineC)]
        L.ohw_pool_set_window_mode.argtypes = [vp, C.c_int]
        L.ohw_pool_create_synthetic.argtypes = [C.POINTER(HParams), C.c_uint32, C.c_char_p, C.c_int, ip, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
        L.ohw_pool_set_force_len.argtypes = [vp, C.c_int]
        L.ohw_pool_set_schedule.argtypes = [vp, C.c_int, C.c_int, C.c_int]
        L.ohw_engine_set_force_len.argtypes = [vp, C.c_int]
        L.ohw_engine_set_beam_size.argtypes = [vp, C.c_int]
        L.ohw_pool_set_beam_size.argtypes = [vp, C.c_int]
        L.ohw_pool_broadcast_note.argtypes = [vp]
        L.ohw_pool_broadcast_note.restype = C.c_char_p
        L.ohw_dsp_rms_db.argtypes = [fp, C.c_int64]
        L.ohw_dsp_rms_db.restype = C.c_float
        L.ohw_dsp_apply_gain.argtypes = [fp, C.c_int64, C.c_float]
        L.ohw_dsp_apply_gain.restype = None
        L.ohw_dsp_normalize_rms.argtypes = [fp, C.c_int64, C.c_float]
        L.ohw_dsp_normalize_rms.restype = None
        L.ohw_dsp_compress.argtypes = [fp, C.c_int64, C.c_uint32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float]
        L.ohw_dsp_compress.restype = None
        L.ohw_dsp_limit.argtypes = [fp, C.c_int64, C.c_uint32, C.c_float, C.c_float]
        L.ohw_dsp_limit.restype = C.c_int64
        L.ohw_dsp_resample_linear.argtypes = [fp, C.c_int64, C.c_uint32, C.c_uint32, fp, C.c_int64]
        L.ohw_dsp_resample_linear.restype = C.c_int64
        L.ohw_dsp_resample_sinc.argtypes = [fp, C.c_int64, C.c_uint32, C.c_uint32, fp, C.c_int64]
        L.ohw_dsp_resample_sinc.restype = C.c_int64
        L.ohw_resampler_create.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.POINTER(vp)]
        L.ohw_tracker_new.argtypes = [C.c_int]
        L.ohw_tracker_new.restype = vp
        L.ohw_tracker_free.argtypes = [vp]
        L.ohw_tracker_free.restype = None
        L.ohw_tracker_add_pending.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
        L.ohw_tracker_add_result.argtypes = [vp, C.c_char_p, C.c_uint64, C.c_uint32, C.c_int, C.c_float]
        L.ohw_tracker_take_ready.argtypes = [vp]
        L.ohw_tracker_ready_get.argtypes = [vp, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_int),
                                            C.POINTER(C.c_float)]
        L.ohw_tracker_reset_dedup.argtypes = [vp]
        L.ohw_tracker_reset_dedup.restype = None
        for fn in (L.ohw_tracker_is_empty, L.ohw_tracker_pending_count, L.ohw_tracker_waiting_count):
            fn.argtypes = [vp]
        L.ohw_tracker_is_pending.argtypes = [vp, C.c_uint64, C.c_uint32]
        L.ohw_extract_chunk.argtypes = [fp, C.c_int64, C.c_int64, C.c_int64, fp, C.c_int64]
        L.ohw_extract_chunk.restype = C.c_int64
        L.ohw_chunk_scheduler_new.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int]
        L.ohw_chunk_scheduler_new.restype = vp
        L.ohw_chunk_scheduler_free.argtypes = [vp]
        L.ohw_chunk_scheduler_free.restype = None
        L.ohw_chunk_scheduler_tick.argtypes = [vp, fp, C.c_int64, C.c_int64, C.POINTER(C.c_uint32), C.POINTER(C.c_int64)]
        L.ohw_chunk_scheduler_tick.restype = C.c_int64
        L.ohw_chunk_scheduler_position.argtypes = [vp]
        L.ohw_chunk_scheduler_position.restype = C.c_int64
        L.ohw_chunk_scheduler_next_id.argtypes = [vp]
        L.ohw_chunk_scheduler_next_id.restype = C.c_uint32
        L.ohw_chunk_scheduler_rejected.argtypes = [vp]
        L.ohw_chunk_scheduler_rejected.restype = C.c_int64
        L.ohw_resampler_free.argtypes = [vp]
        L.ohw_resampler_free.restype = None
        L.ohw_resampler_out_len.argtypes = [vp, C.c_int64]
        L.ohw_resampler_out_len.restype = C.c_int64
        L.ohw_resampler_run.argtypes = [vp, vp, C.c_int64, C.c_int, vp, C.c_int64, C.c_int, vp]
        L.ohw_default_vad_config.argtypes = [C.POINTER(VadConfig)]
        L.ohw_default_vad_config.restype = None
        L.ohw_vad_state_new.argtypes = [C.POINTER(VadConfig), C.c_uint32]
        L.ohw_vad_state_new.restype = vp
        L.ohw_vad_state_free.argtypes = [vp]
        L.ohw_vad_state_free.restype = None
        L.ohw_vad_state_update.argtypes = [vp, C.c_float, C.c_int, C.c_int64, C.POINTER(SpeechSegment)]
        L.ohw_vad_state_is_speech.argtypes = [vp]
        L.ohw_vad_state_speech_start.argtypes = [vp]
        L.ohw_vad_state_speech_start.restype = C.c_int64
        L.ohw_vad_state_reset.argtypes = [vp]
        L.ohw_vad_state_reset.restype = None
        L.ohw_vad_energy_engine.argtypes = [C.c_float, C.POINTER(VadEngineC)]
        L.ohw_vad_energy_engine_free.argtypes = [C.POINTER(VadEngineC)]
        L.ohw_vad_energy_engine_free.restype = None
        L.ohw_vad_run.argtypes = [C.POINTER(VadEngineC), C.POINTER(VadConfig), fp, C.c_int64, C.c_int64, C.POINTER(SpeechSegment), C.c_int64]
        L.ohw_vad_run.restype = C.c_int64
        L.ohw_stream_create.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
        L.ohw_stream_destroy.argtypes = [vp]
        L.ohw_stream_wait.argtypes = [vp, vp]
        L.ohw_stream_sync.argtypes = [vp]
        L.ohw_state_max_batch.argtypes = [vp]
        L.ohw_mel.argtypes = [vp, vp, C.c_int64, ip, C.c_int, C.c_int, C.c_int, fp]
        L.ohw_recording_set.argtypes = [vp, vp, C.c_int64, C.c_int, fp]
        L.ohw_mel_seek.argtypes = [vp, ip, C.c_int, fp]
        L.ohw_recording_set_slot.argtypes = [vp, C.c_int, vp, C.c_int64, C.c_int, fp]
        L.ohw_mel_seek_slots.argtypes = [vp, ip, ip, C.c_int, fp]
        L.ohw_seek_sched_new.argtypes = [C.POINTER(C.c_int64), C.c_int, C.c_int, C.POINTER(vp)]
        L.ohw_seek_sched_round.argtypes = [vp, ip, ip, ip, ip]
        L.ohw_seek_sched_advance.argtypes = [vp, C.c_int, C.c_int]
        L.ohw_seek_sched_free.argtypes = [vp]
        L.ohw_seek_sched_free.restype = None
        L.ohw_engine_transcribe_long_batch.argtypes = [vp, C.POINTER(AudioSpan), ip, C.c_int, C.c_uint32]
        L.ohw_engine_long_batch_quality.argtypes = [vp, C.c_int, C.POINTER(C.POINTER(WindowQuality)), C.POINTER(C.c_int)]
        L.ohw_default_vad_detector.argtypes = [C.POINTER(VadDetector)]
        L.ohw_default_vad_detector.restype = None
        L.ohw_default_chunk_plan.argtypes = [C.POINTER(ChunkPlan)]
        L.ohw_default_chunk_plan.restype = None
        L.ohw_state_vad_frames.argtypes = [vp, vp, C.c_int64, C.c_int, C.POINTER(VadDetector), fp, fp]
        L.ohw_dbg_vad_energy.argtypes = [vp, vp, C.c_int64, C.c_int, fp, C.c_int]
        L.ohw_dbg_vad_floor.argtypes = [vp, fp, C.c_int64, C.POINTER(VadDetector), fp, C.c_int, fp]
        L.ohw_speech_segments_host.argtypes = [fp, C.c_int64, C.c_int, C.c_int64, C.POINTER(VadConfig), C.POINTER(SpeechSegment), C.c_int64]
        L.ohw_speech_segments_host.restype = C.c_int64
        L.ohw_speech_chunks_host.argtypes = [C.POINTER(SpeechSegment), C.c_int64, fp, C.c_int64, C.c_int, C.c_int64, C.POINTER(ChunkPlan),
                                             C.POINTER(SpeechChunk), C.c_int64]
        L.ohw_speech_chunks_host.restype = C.c_int64
        L.ohw_engine_set_vad.argtypes = [vp, C.POINTER(VadConfig), C.POINTER(VadDetector), C.POINTER(ChunkPlan)]
        L.ohw_engine_transcribe_speech.argtypes = [vp, C.POINTER(AudioSpan), C.POINTER(FrameProbs), C.c_int, C.c_uint32]
        L.ohw_engine_transcribe_speech_lang.argtypes = [vp, C.POINTER(AudioSpan), C.POINTER(FrameProbs), ip, C.c_int, C.c_uint32]
        L.ohw_engine_speech_chunks.argtypes = [vp, C.c_int, C.POINTER(C.POINTER(SpeechChunk)), C.POINTER(C.c_int), C.POINTER(C.POINTER(WindowQuality))]
        L.ohw_engine_speech_segments.argtypes = [vp, C.c_int, C.POINTER(C.POINTER(SpeechSegment)), C.POINTER(C.c_int)]
        L.ohw_encode.argtypes = [vp, C.c_int]
        L.ohw_encode_slice.argtypes = [vp, C.c_int, C.c_int, C.c_int]
        L.ohw_detect_language.argtypes = [vp, C.c_int, ip, fp]
        L.ohw_state_ctx.argtypes = [vp]
        L.ohw_state_ctx.restype = vp
        L.ohw_decode.argtypes = [vp, ip, C.c_int, ip, C.c_int, fp]
        L.ohw_default_sample_params.argtypes = [vp, C.POINTER(SampleParams)]
        L.ohw_default_sample_params.restype = None
        L.ohw_sample_greedy_host.argtypes = [vp, C.POINTER(SampleParams), fp, ip, C.c_int, fp]
        L.ohw_greedy.argtypes = [vp, C.POINTER(SampleParams), C.c_int, ip, ip, C.c_int, fp]
        L.ohw_greedy_ex.argtypes = [vp, C.POINTER(SampleParams), C.c_int, C.c_int, C.POINTER(GreedyResult)]
        L.ohw_state_set_logit_bias.argtypes = [vp, fp, C.c_int]
        L.ohw_state_set_batch_invariant.argtypes = [vp, C.c_int]
        L.ohw_state_set_persistent.argtypes = [vp, C.c_int]
        L.ohw_beam_search.argtypes = [vp, C.POINTER(SampleParams), C.c_int, C.c_int, C.c_int, C.POINTER(BeamResult)]
        L.ohw_dbg_sample.argtypes = [vp, C.POINTER(SampleParams), fp, ip, C.c_int, ip, C.c_int, ip, fp, fp]
        L.ohw_decode_active.argtypes = [vp, ip, C.c_int, ip, C.c_int, ip, fp]
        L.ohw_rng_new.argtypes = [C.c_uint32]
        L.ohw_rng_new.restype = vp
        L.ohw_rng_free.argtypes = [vp]
        L.ohw_rng_free.restype = None
        L.ohw_sample_host.argtypes = [vp, C.POINTER(SampleParams), fp, ip, C.c_int, C.c_float, vp, fp, fp]
        L.ohw_rng_uniforms.argtypes = [vp, C.c_int, C.POINTER(C.c_double)]
        L.ohw_rng_discard_draws.argtypes = [vp, C.c_int]
        L.ohw_sample_pass.argtypes = [vp, C.POINTER(SampleParams), C.c_int, C.c_int, C.c_float, ip, C.POINTER(C.c_double), C.POINTER(GreedyResult)]
        L.ohw_dbg_sample_t.argtypes = [vp, C.POINTER(SampleParams), fp, ip, C.c_int, ip, C.c_int, C.c_float, C.POINTER(C.c_double), ip, fp, fp]
        L.ohw_engine_set_fallback_device.argtypes = [vp, C.c_int]
        L.ohw_pool_set_fallback_device.argtypes = [vp, C.c_int]
        L.ohw_default_decode_policy.argtypes = [C.POINTER(DecodePolicy)]
        L.ohw_default_decode_policy.restype = None
        L.ohw_engine_set_decode_policy.argtypes = [vp, C.POINTER(DecodePolicy)]
        L.ohw_engine_last_trace.argtypes = [vp, C.POINTER(ip), C.POINTER(C.c_int)]
        L.ohw_state_timings.argtypes = [vp, C.POINTER(Timings)]
        L.ohw_engine_new.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
        L.ohw_engine_transcribe.argtypes = [vp, fp, C.c_int64, C.c_uint32, C.c_char_p, C.c_size_t, C.c_char_p,
                                            C.POINTER(C.c_uint64), C.POINTER(AudioInfo)]
        L.ohw_engine_set_window_mode.argtypes = [vp, C.c_int]
        L.ohw_engine_set_schedule.argtypes = [vp, C.c_int, C.c_int, C.c_int]
        L.ohw_engine_last_quality.argtypes = [vp, C.POINTER(C.POINTER(WindowQuality)), C.POINTER(C.c_int)]
        L.ohw_engine_last_text.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t)]
        L.ohw_engine_last_tokens.argtypes = [vp, C.POINTER(ip), C.POINTER(C.c_int)]
        L.ohw_engine_benchmark.argtypes = [vp, C.c_float, fp, fp, fp]
        L.ohw_engine_free.argtypes = [vp]
        L.ohw_engine_free.restype = None
        L.ohw_engine_state.argtypes = [vp]
        L.ohw_engine_state.restype = vp
        L.ohw_engine_ctx.argtypes = [vp]
        L.ohw_engine_ctx.restype = vp
        L.ohw_pool_create.argtypes = [C.c_char_p, C.c_char_p, C.c_int, ip, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
        L.ohw_pool_transcribe.argtypes = [vp, fp, C.c_int64, C.c_uint32, C.c_char_p, C.c_size_t, C.c_char_p, C.POINTER(C.c_uint64), C.POINTER(AudioInfo)]
        L.ohw_pool_last_text.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t)]
        L.ohw_pool_last_tokens.argtypes = [vp, C.POINTER(ip), C.POINTER(C.c_int)]
        L.ohw_pool_last_quality.argtypes = [vp, C.POINTER(C.POINTER(WindowQuality)), C.POINTER(C.c_int)]
        L.ohw_pool_set_decode_policy.argtypes = [vp, C.POINTER(DecodePolicy)]
        L.ohw_pool_n_devices.argtypes = [vp]
        L.ohw_pool_broadcast_kind.argtypes = [vp]
        L.ohw_pool_broadcast_kind.restype = C.c_char_p
        L.ohw_pool_engine.argtypes = [vp, C.c_int]
        L.ohw_pool_engine.restype = vp
        L.ohw_pool_free.argtypes = [vp]
        L.ohw_pool_free.restype = None
        L.ohw_state_fetch.argtypes = [vp, C.c_char_p, C.c_int, fp, C.c_int64]
        L.ohw_state_profile_begin.argtypes = [vp, C.c_int]
        L.ohw_state_profile_end.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.ohw_ctx_weight_digest.argtypes = [vp, C.c_int, C.c_char_p, C.POINTER(C.c_uint64)]
        L.ohw_dbg_gemm.argtypes = [C.c_int, vp, vp, vp, vp, C.c_int64, C.c_int64, C.c_int64, C.c_int, vp]
        L.ohw_dbg_attention.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, vp]
        L.ohw_dbg_gemm_small.argtypes = [C.c_int, vp, vp, vp, vp, C.c_int64, C.c_int64, C.c_int64, C.c_int, vp]
        L.ohw_dbg_attention_var.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, ip, ip, vp]
        L.ohw_dbg_cross_attn.argtypes = [C.c_int, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, ip, ip, vp, vp, C.c_int,
                                         C.POINTER(C.c_int), vp]
        L.ohw_dbg_cross_attn_chunk.argtypes = [C.c_int, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, ip, ip, vp]
        L.ohw_state_set_window_prompt.argtypes = [vp, ip, C.c_int, ip, C.c_int]
        L.ohw_state_window_prompt_len.argtypes = [vp, C.c_int]
        L.ohw_state_prefill.argtypes = [vp, C.c_int, ip]
        L.ohw_tokenize_host.argtypes = [C.c_char_p, ip, C.c_int, C.c_char_p, ip, C.c_int]
        L.ohw_tokenize.argtypes = [vp, C.c_char_p, ip, C.c_int]
        L.ohw_prompt_clip_host.argtypes = [ip, C.c_int, C.c_int, ip]
        L.ohw_engine_set_initial_prompt.argtypes = [vp, C.c_char_p]
        L.ohw_engine_set_initial_prompt_tokens.argtypes = [vp, ip, C.c_int]
        L.ohw_pool_set_initial_prompt.argtypes = [vp, C.c_char_p]
        L.ohw_engine_set_carry_context.argtypes = [vp, C.c_int]
        L.ohw_stitch_plan_host.argtypes = [C.c_int64, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.ohw_stitch_seams_host.argtypes = [ip, C.c_int, ip, C.c_int, ip]
        L.ohw_stitch_ranges_host.argtypes = [ip, ip, C.c_int, ip, ip]
        L.ohw_stitch_clip_segment_host.argtypes = [C.POINTER(TokenSpan), C.c_int, C.c_int, C.c_float, C.c_float, C.POINTER(TokenSpan)]
        L.ohw_stitch_seams.argtypes = [C.c_int, ip, C.c_int, ip, C.c_int, ip]
        L.ohw_dbg_stitch.argtypes = [C.c_int, ip, C.c_int, ip, C.c_int, C.c_int, C.c_int32, ip]
        L.ohw_engine_set_stitch.argtypes = [vp, C.c_int]
        L.ohw_engine_stitch.argtypes = [vp]
        L.ohw_engine_last_seams.argtypes = [vp, C.POINTER(C.POINTER(C.c_int32)), C.POINTER(C.c_int)]
        L.ohw_engine_last_window_tokens.argtypes = [vp, C.POINTER(C.POINTER(C.c_int32)), C.POINTER(C.POINTER(C.c_int32)), C.POINTER(C.c_int)]
        L.ohw_state_set_prefill_chunk.argtypes = [vp, C.c_int]
        L.ohw_state_prefill_chunk.argtypes = [vp]
        L.ohw_engine_set_prefill_chunk.argtypes = [vp, C.c_int]
        L.ohw_dbg_cross_attn_chunk_n.argtypes = [C.c_int, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, ip, ip, vp, C.c_int]
        L.ohw_pool_set_carry_context.argtypes = [vp, C.c_int]
        L.ohw_engine_last_context.argtypes = [vp, C.c_int, C.POINTER(C.POINTER(C.c_int32)), C.POINTER(C.c_int)]
        L.ohw_engine_long_batch_context.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.POINTER(C.c_int32)), C.POINTER(C.c_int)]
        L.ohw_carry_step_host.argtypes = [ip, C.POINTER(C.c_int), C.c_int, ip, C.c_int, C.c_float, C.c_int, ip, C.POINTER(C.c_int)]
        L.ohw_dbg_self_attn.argtypes = [C.c_int, vp, vp, vp, ip, vp, C.c_int, C.c_int, C.c_int, C.c_int, ip, C.POINTER(C.c_int), vp]
        L.ohw_dbg_dec_gemm.argtypes = [C.POINTER(DbgDecGemmIO), vp]
        L.ohw_dbg_enc_gemm.argtypes = [C.POINTER(DbgEncGemmIO), vp]
        L.ohw_dbg_embed.argtypes = [C.c_int, vp, C.c_int, vp, C.c_int, ip, ip, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]
        L.ohw_dbg_layernorm.argtypes = [C.c_int, vp, vp, vp, vp, C.c_int64, C.c_int, C.c_int, vp]
        L.ohw_dbg_logits_rows.argtypes = [C.POINTER(DbgLogitsRowsIO), vp]
        L.ohw_state_score.argtypes = [vp, C.POINTER(SampleParams), ip, C.c_int, ip, C.c_int, vp, ip, ip]
        L.ohw_state_set_score_buffers.argtypes = [vp, C.c_int]
        L.ohw_token_score_host.argtypes = [fp, C.c_int, C.c_int, C.c_int, C.POINTER(TokenScore)]
        L.ohw_token_prob_host.argtypes = [C.POINTER(TokenScore), fp, fp, fp]
        L.ohw_word_probs_host.argtypes = [fp, ip, C.c_int, fp]
        L.ohw_dbg_token_score.argtypes = [vp, fp, C.c_int, C.c_int64, C.c_int, C.c_int, ip, ip, C.c_int, C.c_int, C.c_int, C.c_int, vp]
        L.ohw_state_set_audio_ctx.argtypes = [vp, C.c_int]
        L.ohw_state_audio_ctx.argtypes = [vp]
        L.ohw_audio_ctx_for.argtypes = [C.c_int64]
        L.ohw_audio_ctx_for.restype = C.c_int32
        L.ohw_engine_set_audio_ctx.argtypes = [vp, C.c_int]
        L.ohw_pool_set_audio_ctx.argtypes = [vp, C.c_int]
        L.ohw_state_set_window_ctx.argtypes = [vp, C.POINTER(C.c_int32), C.c_int]
        L.ohw_state_window_ctx.argtypes = [vp, C.c_int]
        L.ohw_state_set_packed_encoder.argtypes = [vp, C.c_int]
        L.ohw_state_packed_encoder.argtypes = [vp]
        L.ohw_engine_set_packed_encoder.argtypes = [vp, C.c_int]
        L.ohw_pool_set_packed_encoder.argtypes = [vp, C.c_int]
        L.ohw_dbg_poison.argtypes = [vp, C.c_char_p]
        L.ohw_engine_transcribe_batch.argtypes = [vp, C.POINTER(AudioSpan), C.c_int, C.c_uint32]
        L.ohw_engine_batch_result.argtypes = [vp, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(C.POINTER(C.c_int32)),
                                              C.POINTER(C.c_int), C.POINTER(C.POINTER(WindowQuality)), C.c_char_p]
        L.ohw_batch_plan.argtypes = [C.POINTER(C.c_int64), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                     C.POINTER(C.c_int32)]
        L.ohw_engine_set_detect_language.argtypes = [vp, C.c_int]
        L.ohw_engine_last_language.argtypes = [vp, ip, fp]
        L.ohw_engine_transcribe_batch_lang.argtypes = [vp, C.POINTER(AudioSpan), ip, C.c_int, C.c_uint32]
        L.ohw_pool_set_detect_language.argtypes = [vp, C.c_int]
        L.ohw_state_set_window_lang.argtypes = [vp, C.POINTER(C.c_int32), C.c_int]
        L.ohw_state_detect_window_lang.argtypes = [vp, C.c_int]
        L.ohw_state_window_lang.argtypes = [vp, C.c_int, ip, fp]
        L.ohw_lang_pick_host.argtypes = [fp, C.POINTER(SpecialTokens), ip, fp]
        L.ohw_dbg_lang_pick.argtypes = [vp, fp, C.c_int, ip, fp]
        L.ohw_dbg_counter.argtypes = [vp, C.c_char_p]
        L.ohw_phrase_table_build_host.argtypes = [ip, ip, fp, C.c_int, C.c_int, vp]
        L.ohw_phrase_boost_host.argtypes = [vp, ip, C.c_int, fp, C.c_int]
        L.ohw_state_set_phrase_table.argtypes = [vp, ip, ip, fp, C.c_int]
        L.ohw_state_phrase_count.argtypes = [vp]
        L.ohw_dbg_phrase_boost.argtypes = [vp, fp, C.c_int, C.c_int64, C.c_int, ip, C.c_int, ip, ip, vp]
        L.ohw_engine_set_hot_phrases.argtypes = [vp, C.POINTER(C.c_char_p), fp, C.c_int]
        L.ohw_engine_set_hot_phrases_tokens.argtypes = [vp, ip, ip, fp, C.c_int]
        L.ohw_pool_set_hot_phrases.argtypes = [vp, C.POINTER(C.c_char_p), fp, C.c_int]
        L.ohw_repeat_rule_host.argtypes = [C.c_float, C.c_int, ip, C.c_int, fp, C.c_int, C.c_int]
        L.ohw_state_set_repeat_rule.argtypes = [vp, C.c_float, C.c_int]
        L.ohw_state_repeat_rule.argtypes = [vp, fp, C.POINTER(C.c_int)]
        L.ohw_dbg_repeat_rule.argtypes = [vp, fp, C.c_int, C.c_int64, C.c_int, ip, C.c_int, ip, ip, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int]
        L.ohw_engine_set_repetition.argtypes = [vp, C.c_float, C.c_int]
        L.ohw_pool_set_repetition.argtypes = [vp, C.c_float, C.c_int]
        L.ohw_command_table_build_host.argtypes = [ip, ip, C.c_int, C.c_int, vp]
        L.ohw_command_rule_host.argtypes = [vp, C.c_float, ip, C.c_int, fp, C.c_int, C.c_int, fp]
        L.ohw_command_match_host.argtypes = [vp, ip, C.c_int]
        L.ohw_state_set_command_table.argtypes = [vp, ip, ip, C.c_int, C.c_float]
        L.ohw_state_command_count.argtypes = [vp]
        L.ohw_state_command_list_logprob.argtypes = [vp, C.c_int, fp]
        L.ohw_dbg_command_rule.argtypes = [vp, fp, C.c_int, C.c_int64, C.c_int, ip, C.c_int, ip, ip, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, vp, fp]
        L.ohw_engine_set_commands.argtypes = [vp, C.POINTER(C.c_char_p), C.c_int, C.c_float]
        L.ohw_engine_set_commands_tokens.argtypes = [vp, ip, ip, C.c_int, C.c_float]
        L.ohw_pool_set_commands.argtypes = [vp, C.POINTER(C.c_char_p), C.c_int, C.c_float]
        L.ohw_engine_last_commands.argtypes = [vp, C.POINTER(C.POINTER(CommandHit)), C.POINTER(C.c_int)]
        L.ohw_engine_batch_commands.argtypes = [vp, C.c_int, C.POINTER(C.POINTER(CommandHit)), C.POINTER(C.c_int)]
        L.ohw_dbg_beam_step.argtypes = [vp, C.POINTER(SampleParams), C.POINTER(DbgBeamIO)]
        L.ohw_beam_search_ex.argtypes = [vp, C.POINTER(SampleParams), C.c_int, C.c_int, C.c_int, C.POINTER(BeamResultEx)]
        L.ohw_dbg_beam_step_ex.argtypes = [vp, C.POINTER(SampleParams), C.POINTER(DbgBeamIOEx)]
        L.ohw_dbg_sample_ex.argtypes = [vp, C.POINTER(SampleParams), C.POINTER(DbgSampleIO)]
        L.ohw_dbg_beam_finish.argtypes = [vp, C.POINTER(BeamFinishIO)]
        L.ohw_beam_finish_host.argtypes = [C.POINTER(BeamFinishIO)]
        L.ohw_state_set_align_heads.argtypes = [vp, C.POINTER(AlignHead), C.c_int]
        L.ohw_state_align.argtypes = [vp, C.POINTER(SampleParams), ip, C.c_int, ip, ip, C.c_int, ip]
        L.ohw_align_reduce_host.argtypes = [fp, C.c_int, C.c_int, C.c_int, C.c_int, fp]
        L.ohw_dtw_host.argtypes = [fp, C.c_int, C.c_int, ip]
        L.ohw_dbg_align_probs.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, ip, C.c_int, fp, vp]
        L.ohw_dbg_align_reduce.argtypes = [C.c_int, fp, C.c_int, C.c_int, C.c_int, C.c_int, fp]
        L.ohw_dbg_dtw.argtypes = [C.c_int, fp, C.c_int, C.c_int, ip]
        ptt, pst = C.POINTER(C.POINTER(TokenTime)), C.POINTER(C.POINTER(SpanTime))
        L.ohw_engine_set_word_timestamps.argtypes = [vp, C.POINTER(AlignHead), C.c_int]
        L.ohw_engine_last_token_times.argtypes = [vp, ptt, C.POINTER(C.c_int)]
        L.ohw_engine_last_words.argtypes = [vp, pst, C.POINTER(C.c_int)]
        L.ohw_engine_last_segments.argtypes = [vp, pst, C.POINTER(C.c_int)]
        L.ohw_engine_batch_times.argtypes = [vp, C.c_int, ptt, C.POINTER(C.c_int), pst, C.POINTER(C.c_int), pst, C.POINTER(C.c_int)]
        L.ohw_word_starts_host.argtypes = [C.c_char_p, ip, C.c_int, ip]
        L.ohw_pool_set_word_timestamps.argtypes = [vp, C.POINTER(AlignHead), C.c_int]
        ptp, pwp, psi, pci = C.POINTER(C.POINTER(TokenProb)), C.POINTER(C.POINTER(WordProb)), C.POINTER(C.POINTER(SegmentInfo)), C.POINTER(C.c_int)
        for who in ("engine", "pool"):
            getattr(L, f"ohw_{who}_set_confidence").argtypes = [vp, C.c_int]
            getattr(L, f"ohw_{who}_last_token_probs").argtypes = [vp, ptp, pci]
            getattr(L, f"ohw_{who}_last_word_probs").argtypes = [vp, pwp, pci]
            getattr(L, f"ohw_{who}_last_segment_info").argtypes = [vp, psi, pci]
        L.ohw_engine_batch_confidence.argtypes = [vp, C.c_int, ptp, pci, pwp, pci, psi, pci]
        L.ohw_engine_score_batch.argtypes = [vp, C.POINTER(AudioSpan), C.c_int, ip, ip, C.POINTER(ScoreResultC)]
        L.ohw_pool_last_token_times.argtypes = [vp, ptt, C.POINTER(C.c_int)]
        L.ohw_pool_last_words.argtypes = [vp, pst, C.POINTER(C.c_int)]
        L.ohw_pool_last_segments.argtypes = [vp, pst, C.POINTER(C.c_int)]
        L.ohw_segments_host.argtypes = [ip, C.c_int, C.POINTER(SpecialTokens), C.c_float, C.c_float, C.POINTER(TokenSpan), C.c_int]
        L.ohw_seq_eval_host.argtypes = [C.POINTER(SpecialTokens), ip, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(SeqEval)]
        L.ohw_needs_fallback_host.argtypes = [C.POINTER(SeqEval), C.POINTER(DecodePolicy), C.c_float, C.c_int]
        L.ohw_best_of_pick_host.argtypes = [C.POINTER(SeqEval), C.c_int, C.POINTER(DecodePolicy), ip]
        L.ohw_sample_pass_n.argtypes = [vp, C.POINTER(SampleParams), C.c_int, C.c_int, C.c_int, C.c_float, ip, C.POINTER(C.c_double), C.POINTER(GreedyResult)]
        L.ohw_dbg_sample_group.argtypes = [vp, C.POINTER(SampleParams), fp, ip, C.c_int, ip, C.c_int, C.c_int, C.c_int, C.c_float,
                                           C.POINTER(C.c_double), ip, ip, fp, fp, ip, ip]
        L.ohw_batch_windows_host.argtypes = [C.c_int, C.c_int, C.c_int]
        L.ohw_engine_set_best_of.argtypes = [vp, C.c_int]
        L.ohw_pool_set_best_of.argtypes = [vp, C.c_int]
        L.ohw_engine_last_candidates.argtypes = [vp, C.POINTER(ip), C.POINTER(C.c_int)]
        L.ohw_engine_last_candidate_logprobs.argtypes = [vp, C.POINTER(fp), C.POINTER(C.c_int)]
        L.ohw_dequantize_host.argtypes = [C.c_int, vp, C.c_int64, fp]
        L.ohw_dbg_dequantize.argtypes = [C.c_int, C.c_int, vp, C.c_int64, fp]
        _lib = L
    return _lib


OHW_LANG_DETECT = -1


def _text_bytes(text) -> bytes:
    b = text.encode("utf-8") if isinstance(text, str) else bytes(text)
    if b"\0" in b:
        raise ValueError("text to tokenize must not contain a NUL byte")
    return b


def tokenize_host(vocab: Sequence[bytes], text, cap: Optional[int] = None) -> List[int]:
    """ohw_tokenize_host: `text` (str or bytes) in ids of `vocab` (entry i has id i).  cap: the output buffer's size (default: one
    token per byte always fits); a text with more tokens than cap raises"""
    b = _text_bytes(text)
    lens = np.asarray([len(v) for v in vocab] or [0], dtype=np.int32)
    cap = max(len(b), 1) if cap is None else int(cap)
    out = np.zeros(max(cap, 1), dtype=np.int32)
    n = lib().ohw_tokenize_host(b"".join(vocab), _ip(lens), len(vocab), b, _ip(out), cap)
    if n < 0:
        _raise(n)
    return [int(t) for t in out[:n]]


def prompt_clip(tokens: Sequence[int], n_text_ctx: int) -> List[int]:
    """ohw_prompt_clip_host: the last n_text_ctx / 2 - 1 tokens of a prompt"""
    a = np.ascontiguousarray(list(tokens) or [0], dtype=np.int32)
    out = np.zeros(a.size, dtype=np.int32)
    n = lib().ohw_prompt_clip_host(_ip(a), len(tokens), int(n_text_ctx), _ip(out))
    if n < 0:
        _raise(n)
    return [int(t) for t in out[:n]]


def carry_step_host(history: Sequence[int], n_text_ctx: int, kept: Sequence[int], kept_temperature: float, max_tokens: int = -1):
    """ohw_carry_step_host: the seek loops' carried-context rule, on the host.  Applies a window's kept pass to `history` (a pass
    kept at T >= 0.5 clears it; the kept tokens, timestamps included, are appended; the last n_text_ctx / 2 stay), then derives the
    next window's context (max_tokens: 0 none, -1 the full cap, n > 0 at most n).  Returns (new history, context)"""
    half = max(int(n_text_ctx) // 2, 1)
    if len(history) > half:
        raise ValueError("carry_step_host: the history holds at most n_text_ctx / 2 tokens")
    h = np.zeros(half, dtype=np.int32)
    h[:len(history)] = list(history)
    nh, nc = C.c_int(len(history)), C.c_int(0)
    k = np.ascontiguousarray(list(kept) or [0], dtype=np.int32)
    out = np.zeros(half, dtype=np.int32)
    _check(lib().ohw_carry_step_host(_ip(h), C.byref(nh), int(n_text_ctx), _ip(k), len(kept), float(kept_temperature), int(max_tokens),
                                     _ip(out), C.byref(nc)))
    return [int(t) for t in h[:nh.value]], [int(t) for t in out[:nc.value]]


def lang_pick_host(row: np.ndarray, tok: "SpecialTokens"):
    """ohw_lang_pick_host (host only): one logits row [n_vocab] -> (id, probs [n_langs]); the definition of the device pick"""
    r = np.ascontiguousarray(row, dtype=np.float32)
    assert r.ndim == 1 and r.size >= tok.sot + 1 + tok.n_langs
    i = C.c_int32(0)
    probs = np.zeros(tok.n_langs, dtype=np.float32)
    _check(lib().ohw_lang_pick_host(_fp(r), C.byref(tok), C.byref(i), _fp(probs)))
    return int(i.value), probs


OHW_ALIGN_MAX_HEADS = 32
ALIGN_SECONDS_PER_INDEX = 0.02      # one encoder position


def align_reduce(p: np.ndarray, n_prompt: int, device: Optional[int] = None) -> np.ndarray:
    """ohw_align_reduce_host (device None; no GPU needed) or ohw_dbg_align_reduce: probabilities [A][n_all][n_keys] -> the
    alignment matrix m [n_all - n_prompt][n_keys] (z-score per head and key, median of 7 along the keys, mean over the heads)"""
    p = np.ascontiguousarray(p, dtype=np.float32)
    assert p.ndim == 3
    A, n_all, n_keys = p.shape
    m = np.zeros((max(n_all - int(n_prompt), 0), n_keys), dtype=np.float32)
    if device is None:
        _check(lib().ohw_align_reduce_host(_fp(p), A, n_all, int(n_prompt), n_keys, _fp(m)))
    else:
        _check(lib().ohw_dbg_align_reduce(int(device), _fp(p), A, n_all, int(n_prompt), n_keys, _fp(m)))
    return m


def dtw(m: np.ndarray, device: Optional[int] = None) -> np.ndarray:
    """ohw_dtw_host (device None; no GPU needed) or ohw_dbg_dtw: m [n][n_keys] -> the key at which the path first enters each row"""
    m = np.ascontiguousarray(m, dtype=np.float32)
    assert m.ndim == 2
    n, n_keys = m.shape
    idx = np.zeros(max(n, 1), dtype=np.int32)
    if device is None:
        _check(lib().ohw_dtw_host(_fp(m), n, n_keys, _ip(idx)))
    else:
        _check(lib().ohw_dbg_dtw(int(device), _fp(m), n, n_keys, _ip(idx)))
    return idx[:n]


SEAM_WORDS = ("left_window", "shift", "matches", "left_cut", "right_cut", "n_left", "n_right", "reserved")


def _stitch_table(windows):
    """token-id lists -> (tokens [W][stride] int32, n_text [W] int32, stride); an int32 array [W][stride] with its counts passes through"""
    if isinstance(windows, tuple):
        tok, n_text = windows
        tok = np.ascontiguousarray(tok, dtype=np.int32)
        return tok, np.ascontiguousarray(n_text, dtype=np.int32), int(tok.shape[1])
    stride = max([len(w) for w in windows] + [1])
    tok = np.zeros((len(windows), stride), dtype=np.int32)
    for i, w in enumerate(windows):
        tok[i, :len(w)] = np.asarray(w, dtype=np.int32)
    return tok, np.asarray([len(w) for w in windows], dtype=np.int32), stride


def stitch_plan_host(n_samples: int, overlap_ms: int):
    """ohw_stitch_plan_host -> (hop in samples, windows); window k covers samples [k * hop, min(n, k * hop + 480000))"""
    hop, nw = C.c_int64(0), C.c_int64(0)
    _check(lib().ohw_stitch_plan_host(int(n_samples), int(overlap_ms), C.byref(hop), C.byref(nw)))
    return int(hop.value), int(nw.value)


def stitch_seams_host(windows) -> np.ndarray:
    """ohw_stitch_seams_host: the seam rule between neighbouring windows' TEXT tokens (lists of ids, or (tokens [W][stride],
    n_text [W])) -> int32 [W - 1][8], the words of SEAM_WORDS.  No GPU needed"""
    tok, n_text, stride = _stitch_table(windows)
    out = np.zeros((max(len(n_text) - 1, 0), 8), dtype=np.int32)
    _check(lib().ohw_stitch_seams_host(_ip(tok), stride, _ip(n_text), len(n_text), _ip(out)))
    return out


def stitch_seams(windows, device: int = 0) -> np.ndarray:
    """ohw_stitch_seams: stitch_seams_host's device twin (stitch_kernel, one workgroup per seam) on host arrays"""
    tok, n_text, stride = _stitch_table(windows)
    out = np.zeros((max(len(n_text) - 1, 0), 8), dtype=np.int32)
    _check(lib().ohw_stitch_seams(int(device), _ip(tok), stride, _ip(n_text), len(n_text), _ip(out)))
    return out


def dbg_stitch(windows, n_guard: int = 0, sentinel: int = -1, device: int = 0) -> np.ndarray:
    """ohw_dbg_stitch: stitch_seams with n_guard sentinel-filled seams behind the output -> int32 [W - 1 + n_guard][8] (rows the
    call never touched, all of them when W <= 1, hold the sentinel)"""
    tok, n_text, stride = _stitch_table(windows)
    out = np.full((max(len(n_text) - 1, 0) + int(n_guard), 8), int(sentinel), dtype=np.int32)
    _check(lib().ohw_dbg_stitch(int(device), _ip(tok), stride, _ip(n_text), len(n_text), int(n_guard), int(sentinel), _ip(out)))
    return out


def stitch_ranges_host(seams, n_text):
    """ohw_stitch_ranges_host: the text-token range [first, end) every window keeps -> list of (first, end)"""
    seams = np.ascontiguousarray(seams, dtype=np.int32).reshape(-1, 8)
    n_text = np.ascontiguousarray(n_text, dtype=np.int32)
    first, end = np.zeros(max(len(n_text), 1), dtype=np.int32), np.zeros(max(len(n_text), 1), dtype=np.int32)
    _check(lib().ohw_stitch_ranges_host(_ip(seams), _ip(n_text), len(n_text), _ip(first), _ip(end)))
    return [(int(a), int(b)) for a, b in zip(first[:len(n_text)], end[:len(n_text)])]


def stitch_clip_segment_host(seg, first: int, end: int, t_seam_left: float, t_seam_right: float):
    """ohw_stitch_clip_segment_host: seg = (first, end, t0, t1) in a window's kept tokens against the range [first, end) ->
    the retained (first, end, t0, t1), or None for a segment wholly outside"""
    a, b = TokenSpan(int(seg[0]), int(seg[1]), float(seg[2]), float(seg[3])), TokenSpan()
    rc = lib().ohw_stitch_clip_segment_host(C.byref(a), int(first), int(end), float(t_seam_left), float(t_seam_right), C.byref(b))
    if rc < 0:
        _check(rc)
    return (b.first, b.end, b.t0, b.t1) if rc == 1 else None


def dbg_align_probs(dtype: int, q_ptr: int, xk_ptr: int, rows: int, n_head: int, t_len: int, n_keys: int, heads: Sequence[int],
                    stream: int = 0) -> np.ndarray:
    """ohw_dbg_align_probs: the tap kernel on device tensors q [rows][64 * n_head], xk [n_head][t_len][64] -> p [len(heads)][rows][t_len]"""
    hd = np.asarray(list(heads), dtype=np.int32)
    out = np.full((len(hd), rows, t_len), np.nan, dtype=np.float32)
    _check(lib().ohw_dbg_align_probs(int(dtype), C.c_void_p(q_ptr), C.c_void_p(xk_ptr), rows, n_head, t_len, n_keys, _ip(hd), len(hd), _fp(out),
                                     C.c_void_p(stream or 0)))
    return out


def token_score_host(row: np.ndarray, eot: int, target: int, n_vocab: Optional[int] = None) -> np.ndarray:
    """ohw_token_score_host (host only): one raw logits row -> a TOKEN_SCORE_DTYPE scalar; n_vocab < len(row) leaves the
    columns behind it as padding"""
    r = np.ascontiguousarray(row, dtype=np.float32)
    out = np.zeros(1, dtype=TOKEN_SCORE_DTYPE)
    _check(lib().ohw_token_score_host(_fp(r), int(r.size if n_vocab is None else n_vocab), int(eot), int(target),
                                      C.cast(out.ctypes.data, C.POINTER(TokenScore))))
    return out[0]


def token_prob_host(score) -> Tuple[float, float, float]:
    """ohw_token_prob_host: one score -> (logprob_text, logprob_all, top_logprob_text) as fp32"""
    s = TokenScore(float(score["logit"]), float(score["lse_text"]), float(score["lse_all"]), int(score["top_id"]), float(score["top_logit"]))
    a, b, c = C.c_float(), C.c_float(), C.c_float()
    _check(lib().ohw_token_prob_host(C.byref(s), C.byref(a), C.byref(b), C.byref(c)))
    return np.float32(a.value), np.float32(b.value), np.float32(c.value)


def word_probs_host(logprob_text, starts) -> np.ndarray:
    """ohw_word_probs_host (host only): one window's text-token log-probabilities and word starts -> one probability per word"""
    lp = np.ascontiguousarray(logprob_text, dtype=np.float32)
    st = np.ascontiguousarray(starts, dtype=np.int32)
    assert lp.size == st.size
    out = np.zeros(max(lp.size, 1), dtype=np.float32)
    n = lib().ohw_word_probs_host(_fp(lp) if lp.size else None, _ip(st) if st.size else None, int(lp.size), _fp(out))
    if n < 0:
        _check(n)
    return out[:n].copy()


def word_starts(token_bytes: Sequence[bytes]) -> List[bool]:
    """ohw_word_starts_host (host only): the bytes of one window's text tokens -> which tokens start a word"""
    lens = np.asarray([len(b) for b in token_bytes], dtype=np.int32)
    out = np.zeros(max(len(lens), 1), dtype=np.int32)
    _check(lib().ohw_word_starts_host(b"".join(token_bytes), _ip(lens) if len(lens) else None, len(lens), _ip(out)))
    return [bool(v) for v in out[:len(lens)]]


def segments_host(tokens: Sequence[int], tok: "SpecialTokens", t_off: float, t_end: float):
    """ohw_segments_host (host only): one window's kept tokens -> [(first, end, t0, t1)], tokens [first, end) of the list"""
    t = np.asarray(list(tokens), dtype=np.int32)
    cap = max(len(t), 1)
    out = (TokenSpan * cap)()
    n = int(lib().ohw_segments_host(_ip(t) if len(t) else None, len(t), C.byref(tok), float(t_off), float(t_end), out, cap))
    if n < 0:
        _raise(n)
    return [(out[i].first, out[i].end, float(out[i].t0), float(out[i].t1)) for i in range(n)]


def seq_eval_host(tok: "SpecialTokens", tokens: Sequence[int], plogs: Sequence[float], seek: int, seek_end: int, n_max: int,
                  no_timestamps: bool = False, window_mode: int = OHW_WINDOW_FIXED) -> SeqEval:
    """ohw_seq_eval_host (host only): the engine's judgement of one sampled sequence (end-of-text last when it was sampled) of the
    window [seek, seek_end) in 10 ms frames"""
    t = np.ascontiguousarray(list(tokens) or [0], dtype=np.int32)
    lp = np.ascontiguousarray(list(plogs) or [0.0], dtype=np.float32)
    ev = SeqEval()
    _check(lib().ohw_seq_eval_host(C.byref(tok), _ip(t), _fp(lp), len(tokens), int(seek), int(seek_end), int(n_max), int(bool(no_timestamps)),
                                   int(window_mode), C.byref(ev)))
    return ev


def batch_windows_host(max_batch: int, beam_size: int = 0, best_of: int = 1) -> int:
    """ohw_batch_windows_host (host only): windows per decode batch, max_batch // max(best_of, beam_size, 1)"""
    n = int(lib().ohw_batch_windows_host(int(max_batch), int(beam_size), int(best_of)))
    if n < 1:
        raise WhisperError(OHW_E_INVALID_ARG, f"batch_windows_host: no batch for max_batch {max_batch}, beam size {beam_size}, best_of {best_of}")
    return n


def best_of_pick_host(evs: Sequence[SeqEval], policy: DecodePolicy) -> int:
    """ohw_best_of_pick_host (host only): which of a best-of rung's judged candidates the engine keeps"""
    arr = (SeqEval * len(evs))(*evs)
    kept = np.zeros(1, dtype=np.int32)
    _check(lib().ohw_best_of_pick_host(arr, len(evs), C.byref(policy), _ip(kept)))
    return int(kept[0])


def needs_fallback_host(ev: SeqEval, policy: DecodePolicy, no_speech_prob: float, is_last: bool) -> bool:
    """ohw_needs_fallback_host (host only): does a pass judged `ev` go to the next temperature?"""
    rc = int(lib().ohw_needs_fallback_host(C.byref(ev), C.byref(policy), float(no_speech_prob), int(bool(is_last))))
    if rc < 0:
        _raise(rc)
    return rc == 1


def _token_times(p, n):
    return [{"id": int(p[i].id), "window": int(p[i].window), "t0": float(p[i].t0), "t1": float(p[i].t1)} for i in range(n)]


def _token_probs(p, n):
    return [{"id": int(p[i].id), "window": int(p[i].window), "logprob_text": float(p[i].logprob_text), "logprob_all": float(p[i].logprob_all),
             "logprob_decode": float(p[i].logprob_decode), "top_id": int(p[i].top_id), "top_logprob_text": float(p[i].top_logprob_text)}
            for i in range(n)]


def _word_probs(p, n, text_bytes: bytes):
    return [{"text": text_bytes[p[i].text_off:p[i].text_off + p[i].text_len].decode("utf-8", "replace"), "text_off": int(p[i].text_off),
             "text_len": int(p[i].text_len), "probability": float(p[i].probability)} for i in range(n)]


def _segment_info(p, n):
    return [{"avg_logprob": float(p[i].avg_logprob_text), "no_speech_prob": float(p[i].no_speech_prob), "temperature": float(p[i].temperature)}
            for i in range(n)]


class _ConfidenceMirror:
    """the confidence accessors WhisperEngine and EnginePool share (ohw_engine_* / ohw_pool_*; include/ohw.h, "confidence in the
    engine"); _WHO names the C prefix"""
    _WHO = "engine"

    def set_confidence(self, on: bool = True):
        """ohw_*_set_confidence: score every kept pass with the unconstrained model (off, the default, frees the buffers)"""
        _check(getattr(lib(), f"ohw_{self._WHO}_set_confidence")(self.h, int(bool(on))))

    def last_token_probs(self):
        """[{id, window, logprob_text, logprob_all, logprob_decode, top_id, top_logprob_text}] per kept text token of the last
        transcribe (empty unless confidence is on)"""
        p, n = C.POINTER(TokenProb)(), C.c_int(0)
        _check(getattr(lib(), f"ohw_{self._WHO}_last_token_probs")(self.h, C.byref(p), C.byref(n)))
        return _token_probs(p, n.value)

    def last_word_probs(self):
        """[{text, text_off, text_len, probability}] per word of the last transcribe; no alignment heads needed"""
        p, n = C.POINTER(WordProb)(), C.c_int(0)
        _check(getattr(lib(), f"ohw_{self._WHO}_last_word_probs")(self.h, C.byref(p), C.byref(n)))
        return _word_probs(p, n.value, self._last_text_bytes())

    def last_segment_info(self):
        """[{avg_logprob, no_speech_prob, temperature}], one per entry of last_segments() while confidence is on"""
        p, n = C.POINTER(SegmentInfo)(), C.c_int(0)
        _check(getattr(lib(), f"ohw_{self._WHO}_last_segment_info")(self.h, C.byref(p), C.byref(n)))
        return _segment_info(p, n.value)


def _spans(p, n, text_bytes: bytes):
    return [{"text": text_bytes[p[i].text_off:p[i].text_off + p[i].text_len].decode("utf-8", "replace"), "text_off": int(p[i].text_off),
             "text_len": int(p[i].text_len), "t0": float(p[i].t0), "t1": float(p[i].t1)} for i in range(n)]


def audio_ctx_for(n_samples: int) -> int:
    """the audio context that covers n_samples of 16 kHz audio - the rule of ohw_audio_ctx_for, restated (no library needed):
    min(1500, round_up(ceil(n_samples / 320) + 32, 64)): 320 samples per encoder position, 0.64 s of headroom, whole key blocks"""
    pos = (max(int(n_samples), 0) + 319) // 320 + 32
    return min(1500, (pos + 63) // 64 * 64)


def _audio_ctx_arg(n) -> int:
    """0 / None (off), n > 0 (fixed) or "auto" / -1 -> the integer ohw_engine_set_audio_ctx takes"""
    if n is None:
        return 0
    if isinstance(n, str):
        if n.strip().lower() == "auto":
            return -1
        n = int(n)
    if int(n) < -1:
        raise ValueError("audio_ctx must be 0 (off), a positive context or \"auto\"")
    return int(n)


def batch_plan(n_samples: Sequence[int], max_batch: int, audio_ctx=0):
    """ohw_batch_plan (host only): (order, ctx, envelopes) - the recordings' indices longest first, each recording's context
    under the engine setting `audio_ctx` (0 / None, n or "auto"), and the envelope of every batch of max_batch"""
    ns = np.asarray(list(n_samples), dtype=np.int64)
    n = int(ns.size)
    order = np.zeros(max(n, 1), dtype=np.int32)
    ctx = np.zeros(max(n, 1), dtype=np.int32)
    env = np.zeros(max((n + max(int(max_batch), 1) - 1) // max(int(max_batch), 1), 1), dtype=np.int32)
    _check(lib().ohw_batch_plan(ns.ctypes.data_as(C.POINTER(C.c_int64)), n, int(max_batch), _audio_ctx_arg(audio_ctx), _ip(order), _ip(ctx),
                                _ip(env)))
    return order[:n].tolist(), ctx[:n].tolist(), env.tolist()


def last_error() -> str:
    return lib().ohw_last_error().decode("utf-8", "replace")


def _raise(code: int, info: Optional[AudioInfo] = None):
    msg = last_error()
    if code == OHW_E_MODEL_NOT_FOUND:
        raise ModelNotFound(code, msg)
    if code == OHW_E_VALIDATION:
        raise ValidationFailed(code, msg, info)
    if code in (OHW_E_LOAD_FAILED, OHW_E_NO_GPU, OHW_E_OOM):
        raise LoadFailed(code, msg)
    raise TranscriptionFailed(code, msg)


def _check(code: int):
    if code != 0:
        _raise(code)


def _fp(a: np.ndarray):
    assert a.dtype == np.float32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _ip(a: np.ndarray):
    assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def validate_audio(samples: np.ndarray, sample_rate: int) -> AudioInfo:
    """validation::validate_audio — raises ValidationFailed with .kind in AUDIO_ERRORS values"""
    s = np.ascontiguousarray(samples, dtype=np.float32)
    info = AudioInfo()
    ptr = _fp(s) if s.size else C.cast(None, C.POINTER(C.c_float))
    rc = lib().ohw_validate_audio(ptr, s.size, sample_rate, C.byref(info))
    if rc != 0:
        raise ValidationFailed(rc, "Audio validation failed: " + AUDIO_ERRORS.get(info.error, "?"), info)
    return info


_QUANT_BLOCK_BYTES = {2: 18, 3: 20, 6: 22, 7: 24, 8: 34}   # ttype -> bytes of one block of 32 values


def _dequantize(ttype: int, blocks, n: int, device: Optional[int]) -> np.ndarray:
    raw = np.ascontiguousarray(np.frombuffer(blocks, np.uint8) if isinstance(blocks, (bytes, bytearray, memoryview)) else blocks)
    out = np.empty(max(int(n), 0), np.float32)
    if ttype in _QUANT_BLOCK_BYTES and raw.nbytes < n // 32 * _QUANT_BLOCK_BYTES[ttype]:
        raise ValueError("block data is shorter than n / 32 blocks")
    src = C.c_void_p(raw.ctypes.data)
    if device is None:
        rc = lib().ohw_dequantize_host(ttype, src, n, _fp(out))
        if rc != 0:
            raise ValueError(f"ohw_dequantize_host: bad arguments (ttype {ttype}, n {n})")
    else:
        _check(lib().ohw_dbg_dequantize(device, ttype, src, n, _fp(out)))
    return out


def dequantize_host(ttype: int, blocks, n: int) -> np.ndarray:
    """ohw_dequantize_host: n / 32 ggml blocks of ttype 2 Q4_0, 3 Q4_1, 6 Q5_0, 7 Q5_1 or 8 Q8_0 (bytes or a uint8 array) -> n floats;
    no device needed"""
    return _dequantize(ttype, blocks, n, None)


def dbg_dequantize(ttype: int, blocks, n: int, device: int = 0) -> np.ndarray:
    """ohw_dbg_dequantize: the same through the loader's kernel on `device`"""
    return _dequantize(ttype, blocks, n, device)


def lang_id_to_code(i: int) -> str:
    return lib().ohw_lang_id_to_code(i).decode()


def lang_code_to_id(code: str) -> int:
    return int(lib().ohw_lang_code_to_id(code.encode()))


class Context:
    """ohw_ctx: the model resident in HBM"""

    def __init__(self, handle):
        self.h = C.c_void_p(handle)
        self.hp = HParams()
        self.tok = SpecialTokens()
        _check(lib().ohw_ctx_info(self.h, C.byref(self.hp), C.byref(self.tok)))

    @classmethod
    def from_file(cls, path: str, device: int = 0, dtype: int = OHW_DTYPE_BF16) -> "Context":
        h = C.c_void_p()
        _check(lib().ohw_ctx_create(path.encode(), device, dtype, C.byref(h)))
        return cls(h.value)

    @classmethod
    def synthetic(cls, hparams: Sequence[int], seed: int = 1234, device: int = 0, dtype: int = OHW_DTYPE_BF16) -> "Context":
        hp = HParams(*[int(x) for x in hparams])
        h = C.c_void_p()
        _check(lib().ohw_ctx_create_synthetic(C.byref(hp), seed, device, dtype, C.byref(h)))
        return cls(h.value)

    @classmethod
    def shell(cls, hparams: Sequence[int], device: int = 0, dtype: int = OHW_DTYPE_BF16) -> "Context":
        """every buffer allocated, no weights: the receiving end of a weight broadcast (import_blob)"""
        hp = HParams(*[int(x) for x in hparams])
        h = C.c_void_p()
        _check(lib().ohw_ctx_create_shell(C.byref(hp), device, dtype, C.byref(h)))
        return cls(h.value)

    @property
    def dtype(self) -> int:
        return int(lib().ohw_ctx_dtype(self.h))

    def blob_size(self) -> int:
        return int(lib().ohw_ctx_blob_size(self.h))

    def export_blob(self, dst_device_ptr: int, capacity: int):
        _check(lib().ohw_ctx_blob_export(self.h, C.c_void_p(dst_device_ptr), capacity))

    def import_blob(self, src_device_ptr: int, nbytes: int):
        _check(lib().ohw_ctx_blob_import(self.h, C.c_void_p(src_device_ptr), nbytes))

    def default_params(self) -> SampleParams:
        p = SampleParams()
        lib().ohw_default_sample_params(self.h, C.byref(p))
        return p

    def weight_digests(self) -> dict:
        """name -> 64-bit digest of every resident weight buffer"""
        out, i = {}, 0
        name = C.create_string_buffer(64)
        d = C.c_uint64(0)
        while lib().ohw_ctx_weight_digest(self.h, i, name, C.byref(d)) == 0:
            out[name.value.decode()] = int(d.value)
            i += 1
        return out

    def token_text(self, i: int) -> bytes:
        s = C.c_char_p()
        n = lib().ohw_token_text(self.h, i, C.byref(s))
        return s.value[:n] if n else b""

    def tokenize(self, text) -> List[int]:
        """ohw_tokenize: `text` (str or bytes) in the model's text tokens"""
        b = _text_bytes(text)
        out = np.zeros(max(len(b), 1), dtype=np.int32)
        n = lib().ohw_tokenize(self.h, b, _ip(out), int(out.size))
        if n < 0:
            _raise(n)
        return [int(t) for t in out[:n]]

    def phrase_table_build(self, phrases: Sequence[Sequence[int]], boosts: Sequence[float]) -> PhraseTable:
        """ohw_phrase_table_build_host with the model's end-of-text id: the trie State.set_phrase_table would put on the device"""
        return phrase_table_build_host(phrases, boosts, int(self.tok.eot))

    def sample_greedy_host(self, p: SampleParams, logits: np.ndarray, cur: List[int]) -> Tuple[int, float]:
        lg = np.ascontiguousarray(logits, dtype=np.float32).copy()
        c = np.asarray(cur if len(cur) else [0], dtype=np.int32)
        lp = C.c_float(0)
        tok = lib().ohw_sample_greedy_host(self.h, C.byref(p), _fp(lg), _ip(c), len(cur), C.byref(lp))
        return int(tok), float(lp.value)

    def sample_host(self, p: SampleParams, logits: np.ndarray, cur: List[int], temperature: float, rng: Optional["HostRng"]):
        """ohw_sample_host -> (token, logprob, no_speech_prob or None)"""
        lg = np.ascontiguousarray(logits, dtype=np.float32).copy()
        c = np.asarray(cur if len(cur) else [0], dtype=np.int32)
        lp, ns = C.c_float(0), C.c_float(-1)
        tok = lib().ohw_sample_host(self.h, C.byref(p), _fp(lg), _ip(c), len(cur), temperature, rng.h if rng else None, C.byref(lp), C.byref(ns))
        return int(tok), float(lp.value), (float(ns.value) if len(cur) == 0 else None)

    def close(self):
        if getattr(self, "h", None):
            lib().ohw_ctx_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HostRng:
    """ohw_rng: the std::mt19937 whisper.cpp's decoders sample with (seed 0 per call)"""
    def __init__(self, seed: int = 0):
        self.h = C.c_void_p(lib().ohw_rng_new(seed))

    def uniforms(self, n: int) -> np.ndarray:
        """ohw_rng_uniforms: the next n draws (canonical doubles) without advancing the generator"""
        out = np.zeros(max(1, n), dtype=np.float64)
        _check(lib().ohw_rng_uniforms(self.h, n, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out[:n]

    def discard_draws(self, n: int):
        """ohw_rng_discard_draws: advance by n draws"""
        _check(lib().ohw_rng_discard_draws(self.h, n))

    def __del__(self):
        try:
            if self.h:
                lib().ohw_rng_free(self.h)
                self.h = None
        except Exception:
            pass


class Stream:
    """HIP stream restricted to CU-mask bits [first_cu, first_cu + n_cu) (n_cu = 0: all CUs); see include/ohw.h"""
    def __init__(self, device: int = 0, first_cu: int = 0, n_cu: int = 0):
        self.h = C.c_void_p()
        _check(lib().ohw_stream_create(device, first_cu, n_cu, C.byref(self.h)))

    @property
    def ptr(self) -> int:
        return self.h.value or 0

    def wait(self, other: "Stream"):
        _check(lib().ohw_stream_wait(self.h, other.h))

    def sync(self):
        _check(lib().ohw_stream_sync(self.h))

    def close(self):
        if self.h:
            lib().ohw_stream_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SeekSched:
    """ohw_seek_sched (host only): which recordings run a window in each round of the long-form batch, and where.  round() ->
    [(rec, slot, seek, fresh)] in slot order ([] when every recording has ended); advance(b, seek_delta) once per entry"""

    def __init__(self, n_samples: Sequence[int], max_batch: int):
        ns = np.ascontiguousarray(list(n_samples), dtype=np.int64)
        self.max_batch = int(max_batch)
        h = C.c_void_p()
        _check(lib().ohw_seek_sched_new(ns.ctypes.data_as(C.POINTER(C.c_int64)), len(ns), self.max_batch, C.byref(h)))
        self.h = h

    def round(self):
        a = [np.zeros(max(1, self.max_batch), dtype=np.int32) for _ in range(4)]
        n = int(lib().ohw_seek_sched_round(self.h, *[_ip(x) for x in a]))
        if n < 0:
            _raise(OHW_E_INVALID_ARG)
        return [tuple(int(x[b]) for x in a) for b in range(n)]

    def advance(self, b: int, seek_delta: int):
        _check(lib().ohw_seek_sched_advance(self.h, int(b), int(seek_delta)))

    def close(self):
        if getattr(self, "h", None):
            lib().ohw_seek_sched_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class State:
    """ohw_state: activations + KV caches for up to max_batch 30 s windows"""

    def __init__(self, ctx: Context, max_batch: int = 1):
        self.ctx = ctx
        h = C.c_void_p()
        _check(lib().ohw_state_create(ctx.h, max_batch, C.byref(h)))
        self.h = h
        self.max_batch = max_batch
        self._align_heads = 0
        self._align_shape = []

    def close(self):
        if getattr(self, "h", None):
            lib().ohw_state_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr: Optional[int]):
        _check(lib().ohw_state_set_stream(self.h, C.c_void_p(stream_ptr or 0)))

    def counter(self, name: str) -> int:
        """ohw_dbg_counter: step_captures, beam_captures, step_graphs, beam_graphs, persist_launches, enc_rows, and the decoder
        step's kernel-variant tally (dec_gemm.*, xattn.*, self_attn.*: the names are listed in include/ohw.h)"""
        v = int(lib().ohw_dbg_counter(self.h, name.encode()))
        if v < 0:
            raise ValueError(name)
        return v

    def mel(self, pcm: np.ndarray, n_samples: Optional[Sequence[int]] = None, mode: int = OHW_MEL_REFLECT, want: bool = True):
        """pcm: [B][stride] float32 host array"""
        pcm = np.ascontiguousarray(np.atleast_2d(pcm), dtype=np.float32)
        B, stride = pcm.shape
        ns = np.asarray(n_samples if n_samples is not None else [min(stride, CHUNK_SAMPLES)] * B, dtype=np.int32)
        out = np.empty((B, self.ctx.hp.n_mels, CHUNK_FRAMES), dtype=np.float32) if want else None
        _check(lib().ohw_mel(self.h, pcm.ctypes.data_as(C.c_void_p), stride, _ip(ns), B, 0, mode,
                             _fp(out) if want else C.cast(None, C.POINTER(C.c_float))))
        return out

    def vad_frames(self, pcm, n: Optional[int] = None, detector: Optional[VadDetector] = None):
        """ohw_state_vad_frames: (probabilities [ceil(n / 160)] float32, noise floor in dB) of a recording, one value per 10 ms
        frame, by the device detector (this project's own spectral rule, not Silero).  pcm: a host float32 array, or - with n -
        the address of n samples resident in HBM"""
        on_device = isinstance(pcm, int)
        if on_device:
            ptr, n = C.c_void_p(pcm), int(n)
        else:
            x = np.ascontiguousarray(pcm, dtype=np.float32)
            ptr, n = x.ctypes.data_as(C.c_void_p), x.size if n is None else int(n)
        out = np.empty(max((n + 159) // 160, 0), dtype=np.float32)
        fl = C.c_float(0.0)
        _check(lib().ohw_state_vad_frames(self.h, ptr, n, int(on_device), C.byref(detector) if detector is not None else None,
                                          _fp(out) if out.size else C.cast(None, C.POINTER(C.c_float)), C.byref(fl)))
        return out, float(fl.value)

    def dbg_vad_energy(self, pcm, n: Optional[int] = None, guard: int = 16):
        """ohw_dbg_vad_energy: the band energies e [ceil(n / 160) + guard] of vad_band_kernel (the guard holds
        OHW_DBG_SENTINEL_F32); pcm as in vad_frames"""
        on_device = isinstance(pcm, int)
        if on_device:
            ptr, n = C.c_void_p(pcm), int(n)
        else:
            x = np.ascontiguousarray(pcm, dtype=np.float32)
            ptr, n = x.ctypes.data_as(C.c_void_p), x.size if n is None else int(n)
        out = np.zeros(max((n + 159) // 160, 0) + guard, dtype=np.float32)
        _check(lib().ohw_dbg_vad_energy(self.h, ptr, n, int(on_device), _fp(out), guard))
        return out

    def dbg_vad_floor(self, e: np.ndarray, detector: Optional[VadDetector] = None, guard: int = 16):
        """ohw_dbg_vad_floor: the floor and probability kernels on a caller's e -> (p [len(e) + guard], floor in dB)"""
        x = np.ascontiguousarray(e, dtype=np.float32)
        out = np.zeros(x.size + guard, dtype=np.float32)
        fl = C.c_float(0.0)
        _check(lib().ohw_dbg_vad_floor(self.h, _fp(x) if x.size else C.cast(None, C.POINTER(C.c_float)), x.size,
                                       C.byref(detector) if detector is not None else None, _fp(out), guard, C.byref(fl)))
        return out, float(fl.value)

    def mel_device(self, pcm_ptr: int, stride: int, n_samples: Sequence[int], mode: int = OHW_MEL_REFLECT):
        """pcm already resident in HBM (e.g. a torch tensor's data_ptr())"""
        ns = np.asarray(n_samples, dtype=np.int32)
        _check(lib().ohw_mel(self.h, C.c_void_p(pcm_ptr), stride, _ip(ns), len(ns), 1, mode, C.cast(None, C.POINTER(C.c_float))))

    def recording_set(self, pcm: np.ndarray) -> float:
        """ohw_recording_set: the whole recording into the state -> log10 of the largest mel power over all its frames"""
        x = np.ascontiguousarray(pcm, dtype=np.float32)
        mx = C.c_float(0.0)
        _check(lib().ohw_recording_set(self.h, x.ctypes.data_as(C.c_void_p), x.size, 0, C.byref(mx)))
        return float(mx.value)

    def mel_seek(self, seek_frames: Sequence[int], want: bool = True):
        """ohw_mel_seek: windows [seek, seek + 3000) of the recording-wide spectrogram -> [B][n_mels][3000] (or None)"""
        sk = np.asarray(seek_frames, dtype=np.int32)
        out = np.empty((len(sk), self.ctx.hp.n_mels, CHUNK_FRAMES), dtype=np.float32) if want else None
        _check(lib().ohw_mel_seek(self.h, _ip(sk), len(sk), _fp(out) if want else C.cast(None, C.POINTER(C.c_float))))
        return out

    def recording_set_slot(self, slot: int, pcm: np.ndarray) -> float:
        """ohw_recording_set_slot: a recording into slot `slot` of the state -> log10 of the largest mel power over its frames"""
        x = np.ascontiguousarray(pcm, dtype=np.float32)
        mx = C.c_float(0.0)
        _check(lib().ohw_recording_set_slot(self.h, int(slot), x.ctypes.data_as(C.c_void_p), x.size, 0, C.byref(mx)))
        return float(mx.value)

    def mel_seek_slots(self, slots: Sequence[int], seek_frames: Sequence[int], want: bool = True):
        """ohw_mel_seek_slots: window b = frames [seek_frames[b], +3000) of the recording in slots[b] -> [B][n_mels][3000] (or None)"""
        sl = np.asarray(slots, dtype=np.int32)
        sk = np.asarray(seek_frames, dtype=np.int32)
        if sl.shape != sk.shape:
            raise ValueError("mel_seek_slots: one seek per slot entry")
        out = np.empty((len(sk), self.ctx.hp.n_mels, CHUNK_FRAMES), dtype=np.float32) if want else None
        _check(lib().ohw_mel_seek_slots(self.h, _ip(sl), _ip(sk), len(sk), _fp(out) if want else C.cast(None, C.POINTER(C.c_float))))
        return out

    def encode(self, batch: int):
        _check(lib().ohw_encode(self.h, batch))

    def encode_slice(self, batch: int, first: int, total: int):
        """encoder + cross K/V of the last mel's `batch` windows into windows [first, first + batch) of a decode batch of `total`"""
        _check(lib().ohw_encode_slice(self.h, batch, first, total))

    def detect_language(self, batch: int):
        """(lang_ids [B], probs [B][n_langs]) for the windows of the last encode"""
        ids = np.zeros(batch, dtype=np.int32)
        probs = np.zeros((batch, self.ctx.tok.n_langs), dtype=np.float32)
        _check(lib().ohw_detect_language(self.h, batch, _ip(ids), _fp(probs)))
        return ids, probs

    def decode(self, tokens: np.ndarray, n_past: Sequence[int]) -> np.ndarray:
        """tokens [B][n_new] -> logits [B][n_vocab] of the last fed position"""
        t = np.ascontiguousarray(np.atleast_2d(tokens), dtype=np.int32)
        B, n_new = t.shape
        npast = np.asarray(n_past, dtype=np.int32)
        out = np.empty((B, self.ctx.hp.n_vocab), dtype=np.float32)
        _check(lib().ohw_decode(self.h, _ip(t), n_new, _ip(npast), B, _fp(out)))
        return out

    def decode_active(self, tokens: np.ndarray, n_past: Sequence[int], active: Sequence[int]) -> np.ndarray:
        """ohw_decode_active: as decode(), only the windows with active[b] != 0 (the other rows of the result are zero)"""
        t = np.ascontiguousarray(np.atleast_2d(tokens), dtype=np.int32)
        B, n_new = t.shape
        npast = np.asarray(n_past, dtype=np.int32)
        act = np.asarray(active, dtype=np.int32)
        out = np.zeros((B, self.ctx.hp.n_vocab), dtype=np.float32)
        _check(lib().ohw_decode_active(self.h, _ip(t), n_new, _ip(npast), B, _ip(act), _fp(out)))
        return out

    def greedy(self, batch: int, p: Optional[SampleParams] = None):
        """device-resident greedy loop -> (list of token lists, sum_logprob[B])"""
        p = p or self.ctx.default_params()
        cap = self.ctx.hp.n_text_ctx
        toks = np.zeros((batch, cap), dtype=np.int32)
        nt = np.zeros(batch, dtype=np.int32)
        slp = np.zeros(batch, dtype=np.float32)
        _check(lib().ohw_greedy(self.h, C.byref(p), batch, _ip(toks), _ip(nt), cap, _fp(slp)))
        return [[int(x) for x in toks[b, :nt[b]]] for b in range(batch)], slp

    def greedy_ex(self, batch: int, p: Optional[SampleParams] = None):
        """ohw_greedy_ex -> list of dict(tokens, logprobs [n (+1 with the end-of-text token's)], ended_by_eot, no_speech_prob)"""
        p = p or self.ctx.default_params()
        cap = self.ctx.hp.n_text_ctx
        toks = np.zeros((batch, cap), dtype=np.int32)
        nt = np.zeros(batch, dtype=np.int32)
        slp = np.zeros(batch, dtype=np.float32)
        lps = np.zeros((batch, cap + 1), dtype=np.float32)
        eot = np.zeros(batch, dtype=np.int32)
        nsp = np.zeros(batch, dtype=np.float32)
        r = GreedyResult(_ip(toks), _ip(nt), _fp(slp), _fp(lps), _ip(eot), _fp(nsp))
        _check(lib().ohw_greedy_ex(self.h, C.byref(p), batch, cap, C.byref(r)))
        return [{"tokens": [int(x) for x in toks[b, :nt[b]]], "logprobs": lps[b, :nt[b] + (1 if eot[b] else 0)].copy(),
                 "ended_by_eot": bool(eot[b]), "no_speech_prob": float(nsp[b]), "sum_logprob": float(slp[b])} for b in range(batch)]

    def beam_search(self, n_windows: int, beam_size: int = 5, p: Optional[SampleParams] = None):
        """ohw_beam_search for the windows of the last encode -> [dict(tokens, sum_logprob, n_finished)]; the state needs
        max_batch >= n_windows * beam_size"""
        p = p or self.ctx.default_params()
        cap = self.ctx.hp.n_text_ctx
        toks = np.zeros((n_windows, cap), dtype=np.int32)
        nt = np.zeros(n_windows, dtype=np.int32)
        sm = np.zeros(n_windows, dtype=np.float32)
        nf = np.zeros(n_windows, dtype=np.int32)
        r = BeamResult(_ip(toks), _ip(nt), _fp(sm), _ip(nf))
        _check(lib().ohw_beam_search(self.h, C.byref(p), n_windows, beam_size, cap, C.byref(r)))
        return [{"tokens": [int(x) for x in toks[w, :nt[w]]], "sum_logprob": float(sm[w]), "n_finished": int(nf[w])} for w in range(n_windows)]

    def beam_search_ex(self, n_windows: int, beam_size: int = 5, p: Optional[SampleParams] = None):
        """ohw_beam_search_ex: beam_search's result (the same bits) plus what a decode policy judges ->
        [dict(tokens, sum_logprob, n_finished, logprobs (end-of-text's last when ended_by_eot), ended_by_eot, no_speech_prob)]"""
        p = p or self.ctx.default_params()
        cap = self.ctx.hp.n_text_ctx
        toks = np.zeros((n_windows, cap), dtype=np.int32)
        nt = np.zeros(n_windows, dtype=np.int32)
        sm = np.zeros(n_windows, dtype=np.float32)
        nf = np.zeros(n_windows, dtype=np.int32)
        lps = np.zeros((n_windows, cap + 1), dtype=np.float32)
        eot = np.zeros(n_windows, dtype=np.int32)
        nsp = np.zeros(n_windows, dtype=np.float32)
        r = BeamResultEx(_ip(toks), _ip(nt), _fp(sm), _ip(nf), _fp(lps), _ip(eot), _fp(nsp))
        _check(lib().ohw_beam_search_ex(self.h, C.byref(p), n_windows, beam_size, cap, C.byref(r)))
        return [{"tokens": [int(x) for x in toks[w, :nt[w]]], "sum_logprob": float(sm[w]), "n_finished": int(nf[w]),
                 "logprobs": lps[w, :nt[w] + (1 if eot[w] else 0)].copy(), "ended_by_eot": bool(eot[w]), "no_speech_prob": float(nsp[w])}
                for w in range(n_windows)]

    def set_logit_bias(self, bias: Optional[np.ndarray]):
        """additive bias [n_vocab] on every logits row before the filter (None clears it)"""
        if bias is None:
            _check(lib().ohw_state_set_logit_bias(self.h, C.cast(None, C.POINTER(C.c_float)), 0))
        else:
            b = np.ascontiguousarray(bias, dtype=np.float32)
            _check(lib().ohw_state_set_logit_bias(self.h, _fp(b), b.size))

    def set_phrase_table(self, phrases: Optional[Sequence[Sequence[int]]], boosts: Union[float, Sequence[float]] = 1.0):
        """ohw_state_set_phrase_table: hot phrases as token-id lists with a boost each (or one for all); None or [] clears"""
        phrases = [list(p) for p in (phrases or [])]
        bs = [float(boosts)] * len(phrases) if np.isscalar(boosts) else list(boosts)
        toks, off, b = _flat_phrases(phrases, bs)
        _check(lib().ohw_state_set_phrase_table(self.h, _ip(toks), _ip(off), _fp(b), len(phrases)))

    def phrase_count(self) -> int:
        return int(lib().ohw_state_phrase_count(self.h))

    def set_command_table(self, phrases: Optional[Sequence[Sequence[int]]], penalty: float = COMMAND_PENALTY_DEFAULT):
        """ohw_state_set_command_table: a closed list of phrases as token-id lists; every text token that does not continue a listed
        phrase from the window's start is lowered by `penalty` (float("inf"): banned), end-of-text too until a phrase is complete;
        None or [] clears"""
        phrases = [list(p) for p in (phrases or [])]
        toks, off, _ = _flat_phrases(phrases, [0.0] * len(phrases))
        _check(lib().ohw_state_set_command_table(self.h, _ip(toks), _ip(off), len(phrases), float(penalty)))

    def command_count(self) -> int:
        return int(lib().ohw_state_command_count(self.h))

    def command_list_logprob(self, batch: int) -> np.ndarray:
        """ohw_state_command_list_logprob: per window of the last decoding call, log P(a listed phrase starts | text comes next)
        under the unconstrained model, from the window's latest step without a text token"""
        out = np.empty(int(batch), dtype=np.float32)
        _check(lib().ohw_state_command_list_logprob(self.h, int(batch), _fp(out)))
        return out

    def dbg_command_rule(self, logits: np.ndarray, n_vocab: int, histories: np.ndarray, n_cur, done, table: CommandTable, penalty: float, eot: int,
                         row_mul: int = 1, group: int = 1, sentinel: float = -12345.0) -> Tuple[np.ndarray, np.ndarray]:
        """ohw_dbg_command_rule: the kernel once on logits [rows][ld] (a copy comes back whole), histories [entries * group][max_tokens],
        n_cur (None: every history is empty) and done [entries]; launch row r reads history row r * row_mul under entry
        r * row_mul // group -> (logits, list_logprob [entries], `sentinel` where the kernel wrote nothing)"""
        lg, h, nc, dn = _dbg_rule_rows(logits, histories, n_cur, done, group)
        lp = np.full(dn.size, sentinel, dtype=np.float32)
        _check(lib().ohw_dbg_command_rule(self.h, _fp(lg), lg.shape[0], lg.shape[1], int(n_vocab), _ip(h), h.shape[1], None if nc is None else _ip(nc),
                                          _ip(dn), dn.size, int(row_mul), int(group), float(penalty), int(eot), C.byref(table.c), _fp(lp)))
        return lg, lp

    def set_repeat_rule(self, penalty: float = 1.0, ngram: int = 0):
        """ohw_state_set_repeat_rule: repetition penalty (0.01 .. 100; 1.0 = none) and no-repeat n-gram size (0 .. 32; 0 = none)
        on the row's own sampled tokens, in every decoder of this state; the defaults turn the rule off"""
        _check(lib().ohw_state_set_repeat_rule(self.h, float(penalty), int(ngram)))

    def repeat_rule(self) -> Tuple[float, int]:
        """ohw_state_repeat_rule: (penalty, ngram) in effect; (1.0, 0) is off"""
        theta, n = C.c_float(), C.c_int()
        _check(lib().ohw_state_repeat_rule(self.h, C.byref(theta), C.byref(n)))
        return float(theta.value), int(n.value)

    def dbg_repeat_rule(self, logits: np.ndarray, n_vocab: int, histories: np.ndarray, n_cur, done, penalty: float, ngram: int, eot: int,
                        row_mul: int = 1, group: int = 1) -> np.ndarray:
        """ohw_dbg_repeat_rule: the kernel once on logits [rows][ld] (a copy comes back whole), histories [entries * group][max_tokens],
        n_cur (None: every history is empty) and done [entries]; launch row r reads history row r * row_mul under entry r * row_mul // group"""
        lg, h, nc, dn = _dbg_rule_rows(logits, histories, n_cur, done, group)
        _check(lib().ohw_dbg_repeat_rule(self.h, _fp(lg), lg.shape[0], lg.shape[1], int(n_vocab), _ip(h), h.shape[1], None if nc is None else _ip(nc),
                                         _ip(dn), dn.size, int(row_mul), int(group), float(penalty), int(ngram), int(eot)))
        return lg

    def dbg_phrase_boost(self, logits: np.ndarray, n_vocab: int, histories: np.ndarray, n_cur, done, table: PhraseTable) -> np.ndarray:
        """ohw_dbg_phrase_boost: the kernel once on logits [rows][ld] (a copy comes back whole), histories [rows][max_tokens]"""
        lg, h, nc, dn = _dbg_rule_rows(logits, histories, n_cur, done, 1)
        assert nc is not None and dn.size == lg.shape[0]
        _check(lib().ohw_dbg_phrase_boost(self.h, _fp(lg), lg.shape[0], lg.shape[1], int(n_vocab), _ip(h), h.shape[1], _ip(nc), _ip(dn), C.byref(table.c)))
        return lg

    def set_audio_ctx(self, n_ctx: int):
        """ohw_state_set_audio_ctx: encoder positions per window for later mel / encode / decode calls (whisper.cpp's audio_ctx);
        0 or n_audio_ctx = full context"""
        _check(lib().ohw_state_set_audio_ctx(self.h, int(n_ctx)))

    @property
    def audio_ctx(self) -> int:
        return int(lib().ohw_state_audio_ctx(self.h))

    def set_window_ctx(self, n_ctx: Optional[Sequence[int]]):
        """ohw_state_set_window_ctx: one context per window of the next mel / encode, each in 1..audio_ctx (the envelope); None
        clears them.  Layouts stay those of the envelope: fetch returns [batch][audio_ctx][d], window b's first n_ctx[b] rows valid"""
        if n_ctx is None or len(n_ctx) == 0:
            _check(lib().ohw_state_set_window_ctx(self.h, C.cast(None, C.POINTER(C.c_int32)), 0))
            return
        a = np.ascontiguousarray(n_ctx, dtype=np.int32)
        _check(lib().ohw_state_set_window_ctx(self.h, _ip(a), int(a.size)))

    def window_ctx(self, b: int) -> int:
        """ohw_state_window_ctx: the context of decode-batch slot b of the last encode (the envelope when it ran without lengths)"""
        v = int(lib().ohw_state_window_ctx(self.h, int(b)))
        if v < 0:
            raise ValueError(b)
        return v

    def set_packed_encoder(self, on: bool = True):
        """ohw_state_set_packed_encoder: an encode under per-window lengths (set_window_ctx) runs the encoder on sum(n_ctx) rows,
        the windows laid end to end, instead of batch * audio_ctx; same bits, same fetch layouts; no effect without lengths
        (default off, OHW_ENC_PACKED=1 turns it on for new states)"""
        _check(lib().ohw_state_set_packed_encoder(self.h, int(bool(on))))

    @property
    def packed_encoder(self) -> bool:
        return int(lib().ohw_state_packed_encoder(self.h)) == 1

    def set_window_lang(self, lang_ids: Optional[Sequence[int]]):
        """ohw_state_set_window_lang: one language id per decode-batch slot, or OHW_LANG_DETECT (-1) for an entry that
        detect_window_lang() resolves; None clears the table.  While it is set the decodes ignore p.lang_id"""
        if lang_ids is None or len(lang_ids) == 0:
            _check(lib().ohw_state_set_window_lang(self.h, C.cast(None, C.POINTER(C.c_int32)), 0))
            return
        a = np.ascontiguousarray(lang_ids, dtype=np.int32)
        _check(lib().ohw_state_set_window_lang(self.h, _ip(a), int(a.size)))

    def set_window_prompt(self, contexts: Optional[Sequence[Sequence[int]]]):
        """ohw_state_set_window_prompt: the context tokens (text so far) of every decode-batch slot, an empty list for a slot
        without context; None clears the table"""
        if contexts is None:
            _check(lib().ohw_state_set_window_prompt(self.h, C.cast(None, C.POINTER(C.c_int32)), 0, C.cast(None, C.POINTER(C.c_int32)), 0))
            return
        n = np.asarray([len(t) for t in contexts], dtype=np.int32)
        stride = max(1, int(n.max()) if n.size else 1)
        tok = np.zeros((max(1, len(contexts)), stride), dtype=np.int32)
        for b, t in enumerate(contexts):
            tok[b, :len(t)] = np.asarray(t, dtype=np.int32)
        _check(lib().ohw_state_set_window_prompt(self.h, _ip(tok), stride, _ip(n), len(contexts)))

    def window_prompt_len(self, b: int) -> int:
        """ohw_state_window_prompt_len: the positions slot b's context occupies (0, or its tokens + 1)"""
        n = lib().ohw_state_window_prompt_len(self.h, int(b))
        if n < 0:
            raise WhisperError(n, "window_prompt_len: window index out of range")
        return int(n)

    def prefill(self, batch: int, active: Optional[Sequence[int]] = None):
        """ohw_state_prefill: the table's contexts through the decoder; afterwards decode window b from n_past = window_prompt_len(b)"""
        a = None if active is None else np.ascontiguousarray(active, dtype=np.int32)
        _check(lib().ohw_state_prefill(self.h, int(batch), None if a is None else _ip(a)))

    def set_prefill_chunk(self, positions: int):
        """ohw_state_set_prefill_chunk: the prefill feeds the context in chunks of 8 (default) or 16 positions; a table that is set
        is laid out again"""
        _check(lib().ohw_state_set_prefill_chunk(self.h, int(positions)))

    def prefill_chunk(self) -> int:
        return int(lib().ohw_state_prefill_chunk(self.h))

    def detect_window_lang(self, batch: int):
        """ohw_state_detect_window_lang: resolve the table's pending entries for the windows of the last encode, on the device"""
        _check(lib().ohw_state_detect_window_lang(self.h, int(batch)))

    def window_lang(self, batch: int):
        """ohw_state_window_lang -> (ids [B] (-1: still pending), probs [B][n_langs])"""
        ids = np.zeros(batch, dtype=np.int32)
        probs = np.zeros((batch, self.ctx.tok.n_langs), dtype=np.float32)
        _check(lib().ohw_state_window_lang(self.h, int(batch), _ip(ids), _fp(probs)))
        return ids, probs

    def set_align_heads(self, heads: Optional[Sequence[Tuple[int, int]]]):
        """ohw_state_set_align_heads: the (decoder layer, head) pairs the alignment reads; None / empty clears and frees"""
        hs = list(heads) if heads is not None else []
        self._align_heads = len(hs)
        if not hs:
            _check(lib().ohw_state_set_align_heads(self.h, None, 0))
            return
        arr = (AlignHead * len(hs))(*[AlignHead(int(l), int(h)) for l, h in hs])
        _check(lib().ohw_state_set_align_heads(self.h, arr, len(hs)))

    def align(self, tokens: Sequence[Sequence[int]], n_frames: Sequence[int], p: Optional[SampleParams] = None) -> List[np.ndarray]:
        """ohw_state_align for the windows of the last encode: tokens[b] = window b's text tokens (empty: skip the window),
        n_frames[b] its 10 ms frames of real audio -> per window the start index (20 ms units) of every token, then the end of
        the last one ([] for a skipped window).  The state's self K/V is stale afterwards; every decode rewrites it."""
        p = p or self.ctx.default_params()
        B = len(tokens)
        stride = max([len(t) for t in tokens] + [1])
        tk = np.zeros((B, stride), dtype=np.int32)
        nt = np.zeros(B, dtype=np.int32)
        for b, t in enumerate(tokens):
            nt[b] = len(t)
            tk[b, :len(t)] = np.asarray(t, dtype=np.int32)
        nf = np.asarray(list(n_frames), dtype=np.int32)
        assert nf.size == B
        out = np.full((B, stride + 1), -1, dtype=np.int32)
        _check(lib().ohw_state_align(self.h, C.byref(p), _ip(tk), stride, _ip(nt), _ip(nf), B, _ip(out)))
        # what fetch("align_*") needs to shape its result: (prompt length with [no_timestamps], text tokens, n_keys) per window
        n_prompt = 4 if self.ctx.hp.n_vocab >= 51865 else 2
        self._align_shape = [(n_prompt, int(nt[b]), max(1, min(self.window_ctx(b), int(nf[b]) // 2))) for b in range(B)]
        return [out[b, :nt[b] + 1].copy() if nt[b] else np.zeros(0, np.int32) for b in range(B)]

    def set_score_buffers(self, on: int):
        """ohw_state_set_score_buffers: 0 frees the buffers of score(), 1 makes them, 2 also keeps every call's last window's rows
        for fetch("score_logits", batch)"""
        _check(lib().ohw_state_set_score_buffers(self.h, int(on)))

    def score(self, tokens: Sequence[Sequence[int]], n_frames: Optional[Sequence[int]] = None, p: Optional[SampleParams] = None):
        """ohw_state_score for the windows of the last encode: tokens[b] = window b's text tokens (empty: skip the window) -> per
        window a TOKEN_SCORE_DTYPE array of len(tokens[b]) + 1 entries (the last one scores end-of-text; [] for a skipped window).
        With n_frames the alignment runs in the same replay (alignment heads needed) and the result is (scores, start_idx) with
        start_idx as align() returns it.  The state's self K/V is stale afterwards; every decode rewrites it."""
        p = p or self.ctx.default_params()
        B = len(tokens)
        stride = max([len(t) for t in tokens] + [1])
        tk = np.zeros((B, stride), dtype=np.int32)
        nt = np.zeros(B, dtype=np.int32)
        for b, t in enumerate(tokens):
            nt[b] = len(t)
            tk[b, :len(t)] = np.asarray(t, dtype=np.int32)
        sc = np.zeros((B, stride + 1), dtype=TOKEN_SCORE_DTYPE)
        nf = idx = None
        if n_frames is not None:
            nf = np.asarray(list(n_frames), dtype=np.int32)
            assert nf.size == B
            idx = np.full((B, stride + 1), -1, dtype=np.int32)
        _check(lib().ohw_state_score(self.h, C.byref(p), _ip(tk), stride, _ip(nt), B, sc.ctypes.data, None if nf is None else _ip(nf),
                                     None if idx is None else _ip(idx)))
        n_prompt = 4 if self.ctx.hp.n_vocab >= 51865 else 2
        self._score_chunks = (n_prompt + int(nt.max()) + 1 + 7) // 8 if nt.max() > 0 else 0
        scores = [sc[b, :nt[b] + 1].copy() if nt[b] else np.zeros(0, TOKEN_SCORE_DTYPE) for b in range(B)]
        if idx is None:
            return scores
        self._align_shape = [(n_prompt, int(nt[b]), max(1, min(self.window_ctx(b), int(nf[b]) // 2))) for b in range(B)]
        return scores, [idx[b, :nt[b] + 1].copy() if nt[b] else np.zeros(0, np.int32) for b in range(B)]

    def dbg_token_score(self, logits: np.ndarray, n_vocab: int, eot: int, targets, n_all, row0: int, n_prompt: int, cap: int, guard: int = 4):
        """ohw_dbg_token_score: token_score_kernel once on logits [batch * 8][ld] (padding columns as the caller poisoned them),
        targets [batch * 8], n_all [batch] -> TOKEN_SCORE_DTYPE [guard + batch * cap + guard]; what the kernel did not write
        holds OHW_DBG_SENTINEL_*"""
        lg = np.ascontiguousarray(logits, dtype=np.float32)
        assert lg.ndim == 2 and lg.shape[0] % 8 == 0
        batch = lg.shape[0] // 8
        tg = np.ascontiguousarray(targets, dtype=np.int32)
        na = np.ascontiguousarray(n_all, dtype=np.int32)
        assert tg.size == batch * 8 and na.size == batch
        out = np.zeros(batch * cap + 2 * guard, dtype=TOKEN_SCORE_DTYPE)
        _check(lib().ohw_dbg_token_score(self.h, _fp(lg), batch, lg.shape[1], int(n_vocab), int(eot), _ip(tg), _ip(na), int(row0), int(n_prompt),
                                         int(cap), int(guard), out.ctypes.data))
        return out

    def dbg_lang_pick(self, logits: np.ndarray):
        """the DEVICE language pick on caller-supplied rows [B][n_vocab] -> (ids [B], probs [B][n_langs])"""
        lg = np.ascontiguousarray(np.atleast_2d(logits), dtype=np.float32)
        assert lg.shape[1] == self.ctx.hp.n_vocab
        B = lg.shape[0]
        ids = np.zeros(B, dtype=np.int32)
        probs = np.zeros((B, self.ctx.tok.n_langs), dtype=np.float32)
        _check(lib().ohw_dbg_lang_pick(self.h, _fp(lg), B, _ip(ids), _fp(probs)))
        return ids, probs

    @staticmethod
    def dbg_cross_attn_chunk(dtype: int, q_ptr: int, xk_ptr: int, xv_ptr: int, out_ptr: int, windows: int, n_head: int, t_len: int,
                             win_len: Optional[Sequence[int]] = None, done: Optional[Sequence[int]] = None, stream: Optional[int] = None,
                             n_q: int = 8):
        """ohw_dbg_cross_attn_chunk_n: the prefill's cross-attention kernel on device buffers of the caller (n_q = 8 or 16 query rows
        per window; out in activation-tile order, pre-filled by the caller: the rows of a done window keep what they held)"""
        wl = None if win_len is None else np.ascontiguousarray(win_len, dtype=np.int32)
        dn = None if done is None else np.ascontiguousarray(done, dtype=np.int32)
        _check(lib().ohw_dbg_cross_attn_chunk_n(int(dtype), q_ptr, xk_ptr, xv_ptr, out_ptr, int(windows), int(n_head), int(t_len),
                                                None if wl is None else _ip(wl), None if dn is None else _ip(dn), stream, int(n_q)))

    def poison(self, what: str):
        """ohw_dbg_poison (tests): fill the encoder's "qkv" or "att" buffer with NaN"""
        _check(lib().ohw_dbg_poison(self.h, what.encode()))

    def set_persistent(self, on: bool = True):
        """ohw_state_set_persistent: the one-launch decoder step for at most 16 single-token rows (default off: slower than the launches it replaces)"""
        _check(lib().ohw_state_set_persistent(self.h, int(on)))

    def set_batch_invariant(self, on: bool = True):
        """ohw_state_set_batch_invariant: kernel variants picked from n_new alone - a window's result no longer depends on its batch"""
        _check(lib().ohw_state_set_batch_invariant(self.h, int(bool(on))))

    def dbg_sample(self, p: SampleParams, logits: np.ndarray, histories: Sequence[Sequence[int]]):
        """the DEVICE sampler on caller-supplied rows -> (tokens [B], logprobs [B], no_speech_prob [B])"""
        lg = np.ascontiguousarray(np.atleast_2d(logits), dtype=np.float32)
        B = lg.shape[0]
        stride = max(1, max(len(h) for h in histories))
        hist = np.zeros((B, stride), dtype=np.int32)
        nh = np.zeros(B, dtype=np.int32)
        for b, h in enumerate(histories):
            hist[b, :len(h)] = h
            nh[b] = len(h)
        tok = np.zeros(B, dtype=np.int32)
        lp = np.zeros(B, dtype=np.float32)
        ns = np.zeros(B, dtype=np.float32)
        _check(lib().ohw_dbg_sample(self.h, C.byref(p), _fp(lg), _ip(hist), stride, _ip(nh), B, _ip(tok), _fp(lp), _fp(ns)))
        return tok, lp, ns

    def dbg_sample_t(self, p: SampleParams, logits: np.ndarray, histories: Sequence[Sequence[int]], temperature: float,
                     uniforms: Sequence[float]):
        """the DEVICE temperature sampler on caller-supplied rows, one draw per row -> (tokens [B], logprobs [B], no_speech_prob [B])"""
        lg = np.ascontiguousarray(np.atleast_2d(logits), dtype=np.float32)
        B = lg.shape[0]
        stride = max(1, max(len(h) for h in histories))
        hist = np.zeros((B, stride), dtype=np.int32)
        nh = np.zeros(B, dtype=np.int32)
        for b, h in enumerate(histories):
            hist[b, :len(h)] = h
            nh[b] = len(h)
        u = np.ascontiguousarray(uniforms, dtype=np.float64)
        assert u.shape == (B,)
        tok = np.zeros(B, dtype=np.int32)
        lp = np.zeros(B, dtype=np.float32)
        ns = np.zeros(B, dtype=np.float32)
        _check(lib().ohw_dbg_sample_t(self.h, C.byref(p), _fp(lg), _ip(hist), stride, _ip(nh), B, temperature,
                                      u.ctypes.data_as(C.POINTER(C.c_double)), _ip(tok), _fp(lp), _fp(ns)))
        return tok, lp, ns

    def dbg_sample_ex(self, p: SampleParams, logits: np.ndarray, histories: Sequence[Sequence[int]], n_past=None, done=None,
                      advance: int = 0, temperature: float = 0.0, uniforms=None, sum_logprob=None) -> dict:
        """ohw_dbg_sample_ex: ONE sampler launch (temperature 0: the greedy kernel, > 0: the draw) on host rows, the sampler's whole
        output back.  n_past / done / sum_logprob per row (default 0).  -> dict(tokens [B][max_tokens], n_cur, n_past, done,
        sum_logprob, next_tok [B], tok_lp [B][max_tokens + 1], nosp_prob [B], n_done, tickets [B]); what the launch did not write
        holds OHW_DBG_SENTINEL_* (next_tok, tok_lp, nosp_prob, the history slot at n_cur) or its input"""
        lg = np.ascontiguousarray(np.atleast_2d(logits), dtype=np.float32)
        B, MT = lg.shape[0], self.ctx.hp.n_text_ctx
        assert lg.shape == (B, self.ctx.hp.n_vocab) and len(histories) == B, lg.shape
        vec = lambda x, dt: (np.zeros(B, dt) if x is None else np.array(x, dtype=dt, order="C").reshape(B))
        a = dict(tokens=np.zeros((B, MT), np.int32), n_cur=np.array([len(h) for h in histories], np.int32), n_past=vec(n_past, np.int32),
                 done=vec(done, np.int32), sum_logprob=vec(sum_logprob, np.float32), next_tok=np.zeros(B, np.int32),
                 tok_lp=np.zeros((B, MT + 1), np.float32), nosp_prob=np.zeros(B, np.float32), n_done=np.zeros(1, np.int32))
        for b, h in enumerate(histories):
            a["tokens"][b, :min(len(h), MT)] = h[:MT]           # a history too long keeps its length: the entry refuses it
        tickets = np.ones(B, np.uint32)
        u = None if uniforms is None else np.array(uniforms, dtype=np.float64, order="C").reshape(B)
        io = DbgSampleIO(B, int(advance), float(temperature), _fp(lg),
                         C.cast(None, C.POINTER(C.c_double)) if u is None else u.ctypes.data_as(C.POINTER(C.c_double)),
                         *[(_fp(a[n]) if a[n].dtype == np.float32 else _ip(a[n])) for n, _ in DbgSampleIO._fields_[5:-1]],
                         tickets.ctypes.data_as(C.POINTER(C.c_uint32)))
        _check(lib().ohw_dbg_sample_ex(self.h, C.byref(p), C.byref(io)))
        a["n_done"], a["tickets"] = int(a["n_done"][0]), tickets
        return a

    def dbg_beam_step(self, p: SampleParams, K: int, first: bool, state: dict, logits: np.ndarray, side: int = 0) -> dict:
        """ohw_dbg_beam_step: ONE beam step of the device on host data.  state: tokens [R][n_text_ctx], kv_slot [R][n_text_ctx],
        beam_sum [R], n_cur / n_past_w / win_done / fin_cnt [W], fin_tok [R][n_text_ctx], fin_len / fin_sum [R] (R = W * K);
        logits [W][V] when first, else [R][V]; side: the half of the double buffers that holds the input.
        -> the complete next state under the same keys (tokens / kv_slot: the other half), plus cand_tok, cand_lp [R][K + 1],
        next_tok, n_past [R], n_done and tickets [R]; what the step did not write holds OHW_DBG_SENTINEL_*"""
        W = int(np.asarray(state["n_cur"]).size)
        R, Cx, V = W * K, self.ctx.hp.n_text_ctx, self.ctx.hp.n_vocab
        lg = np.ascontiguousarray(logits, dtype=np.float32)
        assert lg.shape == ((W if first else R), V), lg.shape
        i32 = lambda k, shape: np.array(state[k], dtype=np.int32, order="C").reshape(shape)
        f32 = lambda k, shape: np.array(state[k], dtype=np.float32, order="C").reshape(shape)
        a = dict(tokens=i32("tokens", (R, Cx)), kv_slot=i32("kv_slot", (R, Cx)), n_cur=i32("n_cur", W), n_past_w=i32("n_past_w", W),
                 win_done=i32("win_done", W), beam_sum=f32("beam_sum", R), fin_cnt=i32("fin_cnt", W), fin_tok=i32("fin_tok", (R, Cx)),
                 fin_len=i32("fin_len", R), fin_sum=f32("fin_sum", R),
                 cand_tok=np.zeros((R, K + 1), np.int32), cand_lp=np.zeros((R, K + 1), np.float32),
                 tokens_next=np.zeros((R, Cx), np.int32), kv_slot_next=np.zeros((R, Cx), np.int32),
                 next_tok=np.zeros(R, np.int32), n_past=np.zeros(R, np.int32), n_done=np.zeros(1, np.int32))
        tickets = np.ones(R, np.uint32)
        io = DbgBeamIO(int(bool(first)), K, W, side, _fp(lg),
                       *[(_fp(a[n]) if a[n].dtype == np.float32 else _ip(a[n])) for n, _ in DbgBeamIO._fields_[5:-1]],
                       tickets.ctypes.data_as(C.POINTER(C.c_uint32)))
        _check(lib().ohw_dbg_beam_step(self.h, C.byref(p), C.byref(io)))
        out = {k: a[k] for k in ("n_cur", "n_past_w", "win_done", "beam_sum", "fin_cnt", "fin_tok", "fin_len", "fin_sum", "cand_tok",
                                 "cand_lp", "next_tok", "n_past")}
        out["tokens"], out["kv_slot"] = a["tokens_next"], a["kv_slot_next"]
        out["n_done"], out["tickets"] = int(a["n_done"][0]), tickets
        return out

    def dbg_beam_step_ex(self, p: SampleParams, K: int, first: bool, state: dict, logits: np.ndarray, side: int = 0, nosp: bool = True) -> dict:
        """ohw_dbg_beam_step_ex: dbg_beam_step with the log-probability history.  state may also hold plog and fin_plog
        [R][n_text_ctx + 1]; without plog the history pointers are NULL (the kernels touch none of it).
        -> dbg_beam_step's dict, plus plog (the other half) and fin_plog when plog was given, and nosp_prob [W] when nosp"""
        W = int(np.asarray(state["n_cur"]).size)
        R, Cx, V = W * K, self.ctx.hp.n_text_ctx, self.ctx.hp.n_vocab
        lg = np.ascontiguousarray(logits, dtype=np.float32)
        assert lg.shape == ((W if first else R), V), lg.shape
        i32 = lambda k, shape: np.array(state[k], dtype=np.int32, order="C").reshape(shape)
        f32 = lambda k, shape: np.array(state[k], dtype=np.float32, order="C").reshape(shape)
        a = dict(tokens=i32("tokens", (R, Cx)), kv_slot=i32("kv_slot", (R, Cx)), n_cur=i32("n_cur", W), n_past_w=i32("n_past_w", W),
                 win_done=i32("win_done", W), beam_sum=f32("beam_sum", R), fin_cnt=i32("fin_cnt", W), fin_tok=i32("fin_tok", (R, Cx)),
                 fin_len=i32("fin_len", R), fin_sum=f32("fin_sum", R),
                 cand_tok=np.zeros((R, K + 1), np.int32), cand_lp=np.zeros((R, K + 1), np.float32),
                 tokens_next=np.zeros((R, Cx), np.int32), kv_slot_next=np.zeros((R, Cx), np.int32),
                 next_tok=np.zeros(R, np.int32), n_past=np.zeros(R, np.int32), n_done=np.zeros(1, np.int32))
        tickets = np.ones(R, np.uint32)
        base = DbgBeamIO(int(bool(first)), K, W, side, _fp(lg),
                         *[(_fp(a[n]) if a[n].dtype == np.float32 else _ip(a[n])) for n, _ in DbgBeamIO._fields_[5:-1]],
                         tickets.ctypes.data_as(C.POINTER(C.c_uint32)))
        null = C.cast(None, C.POINTER(C.c_float))
        lp = state.get("plog") is not None
        if lp:
            plog, fin_plog = f32("plog", (R, Cx + 1)), f32("fin_plog", (R, Cx + 1))
            plog_next = np.zeros((R, Cx + 1), np.float32)
        nsp = np.zeros(W, np.float32)
        io = DbgBeamIOEx(base, _fp(plog) if lp else null, _fp(plog_next) if lp else null, _fp(fin_plog) if lp else null, _fp(nsp) if nosp else null)
        _check(lib().ohw_dbg_beam_step_ex(self.h, C.byref(p), C.byref(io)))
        out = {k: a[k] for k in ("n_cur", "n_past_w", "win_done", "beam_sum", "fin_cnt", "fin_tok", "fin_len", "fin_sum", "cand_tok",
                                 "cand_lp", "next_tok", "n_past")}
        out["tokens"], out["kv_slot"] = a["tokens_next"], a["kv_slot_next"]
        out["n_done"], out["tickets"] = int(a["n_done"][0]), tickets
        if lp:
            out["plog"], out["fin_plog"] = plog_next, fin_plog
        if nosp:
            out["nosp_prob"] = nsp
        return out

    beam_finish_host = staticmethod(beam_finish_host)

    def dbg_beam_finish(self, K: int, state: dict, max_tokens: Optional[int] = None) -> dict:
        """ohw_dbg_beam_finish: the device's final ranking on a host-supplied pool and live state (beam_finish_host's arguments;
        the rows must be n_text_ctx long)"""
        return _beam_finish(self.h, K, state, max_tokens)

    def sample_pass(self, batch: int, temperature: float, active: Sequence[int], uniforms: np.ndarray, p: Optional[SampleParams] = None):
        """ohw_sample_pass: one temperature pass on the device; uniforms [batch][n_text_ctx] -> greedy_ex's dicts (zeros for
        inactive rows)"""
        p = p or self.ctx.default_params()
        cap = self.ctx.hp.n_text_ctx
        u = np.ascontiguousarray(uniforms, dtype=np.float64)
        assert u.shape == (batch, cap)
        act = np.ascontiguousarray(active, dtype=np.int32)
        toks = np.zeros((batch, cap), dtype=np.int32)
        nt = np.zeros(batch, dtype=np.int32)
        slp = np.zeros(batch, dtype=np.float32)
        lps = np.zeros((batch, cap + 1), dtype=np.float32)
        eot = np.zeros(batch, dtype=np.int32)
        nsp = np.zeros(batch, dtype=np.float32)
        r = GreedyResult(_ip(toks), _ip(nt), _fp(slp), _fp(lps), _ip(eot), _fp(nsp))
        _check(lib().ohw_sample_pass(self.h, C.byref(p), batch, cap, temperature, _ip(act), u.ctypes.data_as(C.POINTER(C.c_double)), C.byref(r)))
        return [{"tokens": [int(x) for x in toks[b, :nt[b]]], "logprobs": lps[b, :nt[b] + (1 if eot[b] else 0)].copy(),
                 "ended_by_eot": bool(eot[b]), "no_speech_prob": float(nsp[b]), "sum_logprob": float(slp[b])} for b in range(batch)]

    def sample_pass_n(self, n_windows: int, best_of: int, temperature: float, active: Sequence[int], uniforms: np.ndarray,
                      p: Optional[SampleParams] = None):
        """ohw_sample_pass_n: one temperature pass with best_of candidates per window; uniforms [n_windows][best_of][n_text_ctx]
        -> sample_pass's dicts, row w * best_of + j = candidate j of window w (zeros for the rows of inactive windows)"""
        p = p or self.ctx.default_params()
        cap = self.ctx.hp.n_text_ctx
        R = n_windows * best_of
        u = np.ascontiguousarray(uniforms, dtype=np.float64)
        assert u.shape == (n_windows, best_of, cap)
        act = np.ascontiguousarray(active, dtype=np.int32)
        assert act.shape == (n_windows,)
        toks = np.zeros((R, cap), dtype=np.int32)
        nt = np.zeros(R, dtype=np.int32)
        slp = np.zeros(R, dtype=np.float32)
        lps = np.zeros((R, cap + 1), dtype=np.float32)
        eot = np.zeros(R, dtype=np.int32)
        nsp = np.zeros(R, dtype=np.float32)
        r = GreedyResult(_ip(toks), _ip(nt), _fp(slp), _fp(lps), _ip(eot), _fp(nsp))
        _check(lib().ohw_sample_pass_n(self.h, C.byref(p), n_windows, best_of, cap, temperature, _ip(act),
                                       u.ctypes.data_as(C.POINTER(C.c_double)), C.byref(r)))
        return [{"tokens": [int(x) for x in toks[b, :nt[b]]], "logprobs": lps[b, :nt[b] + (1 if eot[b] else 0)].copy(),
                 "ended_by_eot": bool(eot[b]), "no_speech_prob": float(nsp[b]), "sum_logprob": float(slp[b])} for b in range(R)]

    def dbg_sample_group(self, p: SampleParams, logits: np.ndarray, histories: Sequence[Sequence[int]], group: int, first: bool,
                         temperature: float, uniforms: Sequence[float], done: Sequence[int]) -> dict:
        """ohw_dbg_sample_group: the group sampler of sample_pass_n once on host data.  histories / uniforms / done per row
        (rows = windows * group); logits [windows][V] when first, else [rows][V] -> tokens, logprobs, no_speech_prob, done,
        n_cur [rows] and win_done [windows]"""
        R = len(histories)
        assert R % group == 0
        W = R // group
        lg = np.ascontiguousarray(np.atleast_2d(logits), dtype=np.float32)
        assert lg.shape[0] == (W if first else R)
        stride = max(1, max(len(h) for h in histories))
        hist = np.zeros((R, stride), dtype=np.int32)
        nh = np.zeros(R, dtype=np.int32)
        for b, h in enumerate(histories):
            hist[b, :len(h)] = h
            nh[b] = len(h)
        u = np.ascontiguousarray(uniforms, dtype=np.float64)
        assert u.shape == (R,)
        dn = np.ascontiguousarray(done, dtype=np.int32).copy()
        assert dn.shape == (R,)
        tok = np.zeros(R, dtype=np.int32)
        lp = np.zeros(R, dtype=np.float32)
        ns = np.zeros(R, dtype=np.float32)
        wd = np.zeros(W, dtype=np.int32)
        nc = np.zeros(R, dtype=np.int32)
        _check(lib().ohw_dbg_sample_group(self.h, C.byref(p), _fp(lg), _ip(hist), stride, _ip(nh), W, group, int(bool(first)), temperature,
                                          u.ctypes.data_as(C.POINTER(C.c_double)), _ip(dn), _ip(tok), _fp(lp), _fp(ns), _ip(wd), _ip(nc)))
        return {"tokens": tok, "logprobs": lp, "no_speech_prob": ns, "done": dn, "win_done": wd, "n_cur": nc}

    def greedy_host_sampler(self, batch: int, p: Optional[SampleParams] = None):
        """the same loop with the HOST owning the sampler: logits cross PCIe every step"""
        p = p or self.ctx.default_params()
        ctx = self.ctx
        prompt = [ctx.tok.sot]
        if ctx.hp.n_vocab >= 51865:
            prompt += [ctx.tok.sot + 1 + p.lang_id, ctx.tok.translate if p.translate else ctx.tok.transcribe]
        if p.no_timestamps:
            prompt.append(ctx.tok.no_timestamps)
        n_max = p.force_len if p.force_len > 0 else p.n_max
        logits = self.decode(np.tile(np.asarray(prompt, np.int32), (batch, 1)), [0] * batch)
        out = [[] for _ in range(batch)]
        done = [False] * batch
        n_past = [len(prompt)] * batch
        feed = [0] * batch
        for _ in range(n_max):
            for b in range(batch):
                if done[b]:
                    continue
                tok, _ = ctx.sample_greedy_host(p, logits[b], out[b])
                if tok == ctx.tok.eot:
                    done[b] = True
                    continue
                out[b].append(tok)
                feed[b] = tok
                if len(out[b]) >= n_max or n_past[b] + 1 >= ctx.hp.n_text_ctx:
                    done[b] = True
            if all(done):
                break
            logits = self.decode(np.asarray(feed, np.int32).reshape(batch, 1), n_past)
            n_past = [n + (0 if done[b] else 1) for b, n in enumerate(n_past)]
        return out

    def profile_begin(self, kernel_class: int):
        _check(lib().ohw_state_profile_begin(self.h, kernel_class))

    def profile_end(self):
        """(launches, total_ms, work) for the class given to profile_begin"""
        n, ms, w = C.c_int64(0), C.c_double(0), C.c_double(0)
        _check(lib().ohw_state_profile_end(self.h, C.byref(n), C.byref(ms), C.byref(w)))
        return int(n.value), float(ms.value), float(w.value)

    def timings(self) -> Timings:
        t = Timings()
        _check(lib().ohw_state_timings(self.h, C.byref(t)))
        return t

    def fetch(self, what: str, batch: int) -> np.ndarray:
        hp = self.ctx.hp
        if what == "logits":
            # the first `batch` decoder rows of the last step, as its sampler saw them (the hot-phrase boost included)
            out = np.empty((batch, hp.n_vocab), dtype=np.float32)
            _check(lib().ohw_state_fetch(self.h, b"logits", batch, _fp(out), out.size))
            return out
        if what in ("align_q", "align_p", "align_m"):
            # window batch - 1 of the last align(): "align_q" [N_all][A][64], "align_p" [A][N_all][n_keys], "align_m" [N][n_keys]
            A = self._align_heads
            if not A or not 1 <= batch <= len(self._align_shape):
                raise WhisperError(OHW_E_INVALID_ARG, f"fetch: window {batch - 1} was not aligned by the last align() of this State")
            n_prompt, n_text, n_keys = self._align_shape[batch - 1]
            n_all = n_prompt + n_text + 1
            out = np.empty(max(A * n_all * hp.n_audio_ctx, n_all * A * 64), dtype=np.float32)
            _check(lib().ohw_state_fetch(self.h, what.encode(), batch, _fp(out), out.size))
            if what == "align_q":
                return out[:n_all * A * 64].reshape(n_all, A, 64).copy()
            if what == "align_p":
                return out[:A * n_all * n_keys].reshape(A, n_all, n_keys).copy()
            return out[:(n_text + 1) * n_keys].reshape(n_text + 1, n_keys).copy()
        if what == "score_logits":
            # window batch - 1 of the last score() under set_score_buffers(2): [n_chunks * 8][n_vocab], row r = position r
            rows = 8 * getattr(self, "_score_chunks", 0)
            if rows == 0:
                raise WhisperError(OHW_E_INVALID_ARG, "fetch: no window was scored by the last score() of this State")
            out = np.empty((rows, hp.n_vocab), dtype=np.float32)
            _check(lib().ohw_state_fetch(self.h, what.encode(), batch, _fp(out), out.size))
            return out
        if what == "sample_slots":
            # the kv_slot table of the last sample_pass_n: batch = its n_windows * best_of rows -> i32 [batch][n_text_ctx]
            out = np.empty((batch, hp.n_text_ctx), dtype=np.float32)
            _check(lib().ohw_state_fetch(self.h, what.encode(), batch, _fp(out), out.size))
            return out.astype(np.int32)
        d, T = hp.n_audio_state, hp.n_audio_ctx
        shape = {"mel": (batch, hp.n_mels, CHUNK_FRAMES), "conv1": (batch, CHUNK_FRAMES, d),
                 "mel_t": (batch, CHUNK_FRAMES + 2, 128)}.get(what, (batch, T, d))
        out = np.empty(shape, dtype=np.float32)
        _check(lib().ohw_state_fetch(self.h, what.encode(), batch, _fp(out), out.size))
        if what not in ("mel", "conv1", "mel_t") and self.audio_ctx < T:
            # the last encode ran a reduced context: the library packed [batch][C][d] into the front of the buffer
            Cn = self.audio_ctx
            out = out.reshape(-1)[:batch * Cn * d].reshape(batch, Cn, d).copy()
        return out


# ---- mirror of the reference's engine types ------------------------------------------------------
@dataclasses.dataclass
class AudioBuffer:
    """reference src/input/audio.rs:55-61"""
    samples: np.ndarray
    sample_rate: int = 16000

    def duration_secs(self) -> float:
        return len(self.samples) / float(self.sample_rate)

    # ---- the reference's AudioBuffer DSP (src/input/audio.rs:86-239), in place, through libohw (host code) ----
    def _buf(self) -> np.ndarray:
        if not (isinstance(self.samples, np.ndarray) and self.samples.dtype == np.float32 and self.samples.flags.c_contiguous
                and self.samples.flags.writeable):
            self.samples = np.array(self.samples, dtype=np.float32, order="C")
        return self.samples

    def rms_db(self) -> float:
        b = self._buf()
        return float(lib().ohw_dsp_rms_db(_fp(b) if b.size else C.cast(None, C.POINTER(C.c_float)), b.size))

    def apply_gain(self, gain_db: float):
        b = self._buf()
        if b.size:
            lib().ohw_dsp_apply_gain(_fp(b), b.size, gain_db)

    def normalize_rms(self, target_db: float):
        b = self._buf()
        if b.size:
            lib().ohw_dsp_normalize_rms(_fp(b), b.size, target_db)

    def compress(self, threshold_db: float, ratio: float, attack_ms: float, release_ms: float, makeup_gain_db: float):
        b = self._buf()
        if b.size:
            lib().ohw_dsp_compress(_fp(b), b.size, self.sample_rate, threshold_db, ratio, attack_ms, release_ms, makeup_gain_db)

    def limit(self, ceiling_db: float, release_ms: float) -> int:
        b = self._buf()
        return int(lib().ohw_dsp_limit(_fp(b), b.size, self.sample_rate, ceiling_db, release_ms)) if b.size else 0

    def preprocess(self, config: Optional["PreprocessConfig"] = None, noise_reduction: bool = False, strength: float = 1.0,
                   denoiser: Optional["Denoiser"] = None):
        """TranscriptionWorker::preprocess_audio (reference src/queue/worker.rs:196-240): noise reduction first and
        independently of the preprocessing switch (needs a Denoiser: the network is the host's), then the chain"""
        b = self._buf()
        cfg = config or default_preprocess_config()
        if not b.size:
            return
        if noise_reduction:
            if denoiser is None:
                raise WhisperError(OHW_E_INVALID_ARG, "noise reduction is enabled but no denoise engine is plugged in")
            _check(lib().ohw_preprocess_audio_ex(_fp(b), b.size, self.sample_rate, C.byref(cfg), 1, strength, C.byref(denoiser.c)))
        else:
            _check(lib().ohw_preprocess_audio(_fp(b), b.size, self.sample_rate, C.byref(cfg)))

    def denoise(self, strength: float, denoiser: "Denoiser"):
        """AudioBuffer::denoise (reference src/input/audio.rs:249-341) with the plugged-in frame processor"""
        b = self._buf()
        if b.size:
            _check(lib().ohw_dsp_denoise(_fp(b), b.size, self.sample_rate, strength, C.byref(denoiser.c)))


class Denoiser:
    """ohw_denoise_engine around a Python callable frame(float32[480]) -> float32[480] (the stand-in for
    nnnoiseless::DenoiseState::process_frame); Denoiser() without a callable is the library's pass-through engine"""

    def __init__(self, process_frame=None, reset=None):
        self.c = DenoiseEngineC()
        self.frames = 0
        if process_frame is None:
            lib().ohw_denoise_passthrough_engine(C.byref(self.c))
            return

        def _frame(_user, out, inp):
            self.frames += 1
            res = np.asarray(process_frame(np.ctypeslib.as_array(inp, shape=(480,)).copy()), dtype=np.float32)
            np.ctypeslib.as_array(out, shape=(480,))[:] = res
            return 1.0

        def _reset(_user):
            if reset:
                reset()
        self._keep = (DENOISE_FRAME_FN(_frame), DENOISE_RESET_FN(_reset))
        self.c.user = None
        self.c.process_frame, self.c.reset = self._keep


def default_preprocess_config() -> PreprocessConfig:
    c = PreprocessConfig()
    lib().ohw_default_preprocess_config(C.byref(c))
    return c


def resample_linear(samples: np.ndarray, from_rate: int, to_rate: int) -> np.ndarray:
    """resample(.., ResamplingQuality::Low) of the reference (src/input/audio.rs:960-990)"""
    x = np.ascontiguousarray(samples, dtype=np.float32)
    if x.size == 0:
        return x.copy()
    n = int(lib().ohw_dsp_resample_linear(_fp(x), x.size, from_rate, to_rate, C.cast(None, C.POINTER(C.c_float)), 0))
    out = np.empty(n, np.float32)
    if n:
        lib().ohw_dsp_resample_linear(_fp(x), x.size, from_rate, to_rate, _fp(out), n)
    return out


def resample_sinc(samples: np.ndarray, from_rate: int, to_rate: int) -> np.ndarray:
    """resample(.., ResamplingQuality::High) of the reference (src/input/audio.rs:1007-1095): rubato's sinc resampler restated"""
    x = np.ascontiguousarray(samples, dtype=np.float32)
    if x.size == 0:
        return x.copy()
    n = int(lib().ohw_dsp_resample_sinc(_fp(x), x.size, from_rate, to_rate, C.cast(None, C.POINTER(C.c_float)), 0))
    out = np.empty(n, np.float32)
    if n:
        lib().ohw_dsp_resample_sinc(_fp(x), x.size, from_rate, to_rate, _fp(out), n)
    return out


class DeviceResampler:
    """ohw_resampler_*: the sinc resampler on the device (same output as resample_sinc up to fp32 summation order)"""
    def __init__(self, from_rate: int, to_rate: int, device: int = 0):
        self.h = C.c_void_p()
        _check(lib().ohw_resampler_create(device, from_rate, to_rate, C.byref(self.h)))

    def out_len(self, n: int) -> int:
        return int(lib().ohw_resampler_out_len(self.h, n))

    def run(self, samples: np.ndarray) -> np.ndarray:
        """host samples in, host samples out"""
        x = np.ascontiguousarray(samples, dtype=np.float32)
        out = np.empty(self.out_len(x.size), np.float32)
        if out.size:
            _check(lib().ohw_resampler_run(self.h, x.ctypes.data_as(C.c_void_p), x.size, 0, out.ctypes.data_as(C.c_void_p), out.size, 0, None))
        return out

    def run_device(self, in_ptr: int, n: int, out_ptr: int, out_cap: int, stream: int = 0) -> int:
        """device pointers (e.g. torch tensors' data_ptr()); asynchronous on `stream`; returns the number of output samples"""
        m = self.out_len(n)
        _check(lib().ohw_resampler_run(self.h, C.c_void_p(in_ptr), n, 1, C.c_void_p(out_ptr), out_cap, 1, C.c_void_p(stream) if stream else None))
        return m

    def close(self):
        if self.h:
            lib().ohw_resampler_free(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001 - interpreter shutdown
            pass


def default_vad_config() -> VadConfig:
    c = VadConfig()
    lib().ohw_default_vad_config(C.byref(c))
    return c


class VadState:
    """reference src/vad/mod.rs:112-250"""
    def __init__(self, config: VadConfig, sample_rate: int = 16000):
        self.h = C.c_void_p(lib().ohw_vad_state_new(C.byref(config), sample_rate))

    def update(self, probability: float, is_speech: bool, chunk_samples: int):
        """the completed (start, end, avg_probability) when speech just ended, else None"""
        seg = SpeechSegment()
        rc = lib().ohw_vad_state_update(self.h, probability, int(is_speech), chunk_samples, C.byref(seg))
        return (int(seg.start), int(seg.end), float(seg.avg_probability)) if rc == 1 else None

    def is_speech(self) -> bool:
        return bool(lib().ohw_vad_state_is_speech(self.h))

    def speech_start(self):
        v = int(lib().ohw_vad_state_speech_start(self.h))
        return None if v < 0 else v

    def reset(self):
        lib().ohw_vad_state_reset(self.h)

    def __del__(self):
        try:
            if self.h:
                lib().ohw_vad_state_free(self.h)
                self.h = None
        except Exception:
            pass


def vad_segments(samples: np.ndarray, config: VadConfig, poll_samples: int = 8000, process=None, energy_threshold_db: float = -40.0):
    """ohw_vad_run over a recording: `process(samples) -> probability` is the VadEngine hook (a Python callable here; the
    built-in energy detector when None).  Returns [(start, end, avg_probability)]."""
    x = np.ascontiguousarray(samples, dtype=np.float32)
    eng = VadEngineC()
    keep = None
    if process is None:
        _check(lib().ohw_vad_energy_engine(energy_threshold_db, C.byref(eng)))
    else:
        def _proc(user, ptr, n, out):
            out[0] = float(process(np.ctypeslib.as_array(ptr, shape=(n,)).copy()))
            return 0
        keep = VAD_PROCESS_FN(_proc)
        eng.process, eng.reset, eng.chunk_size, eng.sample_rate = keep, VAD_RESET_FN(0), 512, 16000
    cap = max(16, x.size // 1600)
    segs = (SpeechSegment * cap)()
    n = int(lib().ohw_vad_run(C.byref(eng), C.byref(config), _fp(x) if x.size else C.cast(None, C.POINTER(C.c_float)), x.size, poll_samples, segs, cap))
    if process is None:
        lib().ohw_vad_energy_engine_free(C.byref(eng))
    if n < 0:
        _check(n)
    return [(int(segs[i].start), int(segs[i].end), float(segs[i].avg_probability)) for i in range(min(n, cap))]


def default_vad_config() -> VadConfig:
    c = VadConfig()
    lib().ohw_default_vad_config(C.byref(c))
    return c


def default_vad_detector() -> VadDetector:
    d = VadDetector()
    lib().ohw_default_vad_detector(C.byref(d))
    return d


def default_chunk_plan() -> ChunkPlan:
    p = ChunkPlan()
    lib().ohw_default_chunk_plan(C.byref(p))
    return p


def speech_segments_host(probs, frame_samples: int, n_samples: int, config: Optional[VadConfig] = None):
    """ohw_speech_segments_host (no GPU): per-frame probabilities -> [(start, end, avg_probability)] in samples, padded and
    clipped.  This project's own rule, modelled on Silero's get_speech_timestamps"""
    p = np.ascontiguousarray(probs, dtype=np.float32)
    cap = p.size // 2 + 1
    segs = (SpeechSegment * cap)()
    n = int(lib().ohw_speech_segments_host(_fp(p) if p.size else C.cast(None, C.POINTER(C.c_float)), p.size, int(frame_samples), int(n_samples),
                                           C.byref(config) if config is not None else None, segs, cap))
    if n < 0:
        raise ValueError("speech_segments_host: bad probabilities or config")
    return [(int(segs[i].start), int(segs[i].end), float(segs[i].avg_probability)) for i in range(min(n, cap))]


def speech_chunks_host(segments, probs, frame_samples: int, n_samples: int, plan: Optional[ChunkPlan] = None):
    """ohw_speech_chunks_host (no GPU): segments [(start, end[, avg])] -> [(start, end, first_segment, n_segments)]"""
    p = np.ascontiguousarray(probs, dtype=np.float32)
    segs = (SpeechSegment * max(len(segments), 1))()
    for i, sg in enumerate(segments):
        segs[i].start, segs[i].end = int(sg[0]), int(sg[1])
        segs[i].avg_probability = float(sg[2]) if len(sg) > 2 else 0.0
    args = (segs, len(segments), _fp(p) if p.size else C.cast(None, C.POINTER(C.c_float)), p.size, int(frame_samples), int(n_samples),
            C.byref(plan) if plan is not None else None)
    n = int(lib().ohw_speech_chunks_host(*args, None, 0))
    if n < 0:
        raise ValueError("speech_chunks_host: bad segments or plan")
    out = (SpeechChunk * max(n, 1))()
    lib().ohw_speech_chunks_host(*args, out, n)
    return [(int(out[i].start), int(out[i].end), int(out[i].first_segment), int(out[i].n_segments)) for i in range(n)]


class EnergyVad:
    """the built-in energy detector as a VadEngine (process(samples) -> probability): ohw_vad_energy_engine.  Not Silero."""
    def __init__(self, threshold_db: float = -40.0):
        self.eng = VadEngineC()
        _check(lib().ohw_vad_energy_engine(threshold_db, C.byref(self.eng)))

    def __call__(self, samples: np.ndarray) -> float:
        x = np.ascontiguousarray(samples, dtype=np.float32)
        out = C.c_float(0.0)
        if self.eng.process(self.eng.user, _fp(x) if x.size else C.cast(None, C.POINTER(C.c_float)), x.size, C.byref(out)) != 0:
            raise WhisperError("vad process failed")
        return float(out.value)

    def close(self):
        if self.eng is not None:
            lib().ohw_vad_energy_engine_free(C.byref(self.eng))
            self.eng = None

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001 - interpreter shutdown
            pass


@dataclasses.dataclass
class TranscriptionResult:
    """reference src/engine/whisper.rs:30-40"""
    text: str
    language: str
    duration_ms: int
    # transcribe_batch only: the recording's times (WhisperEngine.batch_times); token_times and words stay empty unless
    # set_word_timestamps is on
    token_times: list = dataclasses.field(default_factory=list)
    words: list = dataclasses.field(default_factory=list)
    segments: list = dataclasses.field(default_factory=list)
    # the recording's confidence (WhisperEngine.batch_confidence); empty unless set_confidence is on
    token_probs: list = dataclasses.field(default_factory=list)
    word_probs: list = dataclasses.field(default_factory=list)
    segment_info: list = dataclasses.field(default_factory=list)


@dataclasses.dataclass
class BenchmarkResult:
    """reference src/engine/whisper.rs:314-323"""
    overhead_secs: float
    recommended_chunk_interval: float
    test_audio_secs: float


class WhisperEngine(_ConfidenceMirror):
    """Drop-in mirror of the reference's WhisperEngine over libohw.so."""

    def __init__(self, handle):
        self.h = handle
        self.ctx_h = C.c_void_p(lib().ohw_engine_ctx(self.h))
        self.state_h = C.c_void_p(lib().ohw_engine_state(self.h))

    @classmethod
    def new(cls, model_path: str, language: str, translate: bool, use_gpu: bool, device: int = 0,
            dtype: int = OHW_DTYPE_BF16, max_batch: int = 1) -> "WhisperEngine":
        h = C.c_void_p()
        rc = lib().ohw_engine_new(str(model_path).encode(), language.encode(), int(translate), int(use_gpu), device, dtype,
                                  max_batch, C.byref(h))
        if rc != 0:
            _raise(rc)
        return cls(h)

    @classmethod
    def from_config(cls, config: "TranscriptionConfig", data_dir: Optional[str] = None, device: int = 0, dtype: int = OHW_DTYPE_BF16,
                    max_batch: int = 1) -> "WhisperEngine":
        """reference src/engine/whisper.rs:183-201: model = effective_model() parsed as a WhisperModel (anything it does not know:
        Base), path = <data dir>/models/<filename>, use_gpu = device != "cpu" (any case), then new().  `data_dir` stands for
        Config::data_dir() (the platform's ProjectDirs path; default here: $XDG_DATA_HOME or ~/.local/share, then /openhush)."""
        path, use_gpu = config.engine_arguments(data_dir)
        return cls.new(path, config.language, config.translate, use_gpu, device, dtype, max_batch)

    def transcribe(self, audio: AudioBuffer) -> TranscriptionResult:
        s = np.ascontiguousarray(audio.samples, dtype=np.float32)
        buf = C.create_string_buffer(256)
        lang = C.create_string_buffer(8)
        ms = C.c_uint64(0)
        info = AudioInfo()
        ptr = _fp(s) if s.size else C.cast(None, C.POINTER(C.c_float))
        rc = lib().ohw_engine_transcribe(self.h, ptr, s.size, audio.sample_rate, buf, len(buf), lang, C.byref(ms), C.byref(info))
        if rc != 0:
            _raise(rc, info)
        full, n = C.c_char_p(), C.c_size_t(0)
        _check(lib().ohw_engine_last_text(self.h, C.byref(full), C.byref(n)))   # the fixed buffer may have truncated
        text = C.string_at(full, n.value).decode("utf-8", "replace") if n.value else ""
        return TranscriptionResult(text, lang.value.decode(), int(ms.value))

    def state_view(self) -> "State":
        """the engine's own state as a State that does not own it (close() and garbage collection leave the handle alone): what a
        caller scores or inspects with between two transcribes (State.score, counter, fetch)"""
        ctx = Context.__new__(Context)
        ctx.h, ctx.hp, ctx.tok = self.ctx_h, HParams(), SpecialTokens()
        _check(lib().ohw_ctx_info(ctx.h, C.byref(ctx.hp), C.byref(ctx.tok)))
        ctx.close = lambda: None
        st = State.__new__(State)
        st.ctx, st.h, st.max_batch, st._align_heads, st._align_shape = ctx, self.state_h, int(lib().ohw_state_max_batch(self.state_h)), 0, []
        st.close = lambda: None
        return st

    def set_word_timestamps(self, heads: Optional[Sequence[Tuple[int, int]]]):
        """ohw_engine_set_word_timestamps: the (decoder layer, head) pairs to align with; None / empty = off (the default)"""
        hs = list(heads) if heads is not None else []
        if not hs:
            _check(lib().ohw_engine_set_word_timestamps(self.h, None, 0))
            return
        arr = (AlignHead * len(hs))(*[AlignHead(int(l), int(h)) for l, h in hs])
        _check(lib().ohw_engine_set_word_timestamps(self.h, arr, len(hs)))

    def _last_text_bytes(self) -> bytes:
        full, n = C.c_char_p(), C.c_size_t(0)
        _check(lib().ohw_engine_last_text(self.h, C.byref(full), C.byref(n)))
        return C.string_at(full, n.value) if n.value else b""

    def last_token_times(self):
        """[{id, window, t0, t1}] per aligned text token of the last transcribe (empty unless word timestamps are on)"""
        p, n = C.POINTER(TokenTime)(), C.c_int(0)
        _check(lib().ohw_engine_last_token_times(self.h, C.byref(p), C.byref(n)))
        return _token_times(p, n.value)

    def last_words(self):
        """[{text, text_off, text_len, t0, t1}] of the last transcribe; offsets index the UTF-8 bytes of its text"""
        p, n = C.POINTER(SpanTime)(), C.c_int(0)
        _check(lib().ohw_engine_last_words(self.h, C.byref(p), C.byref(n)))
        return _spans(p, n.value, self._last_text_bytes())

    def last_segments(self):
        """the same for the segments between timestamp tokens (always available)"""
        p, n = C.POINTER(SpanTime)(), C.c_int(0)
        _check(lib().ohw_engine_last_segments(self.h, C.byref(p), C.byref(n)))
        return _spans(p, n.value, self._last_text_bytes())

    def batch_times(self, i: int):
        """(token_times, words, segments) of recording i of the last transcribe_batch"""
        tp, tn = C.POINTER(TokenTime)(), C.c_int(0)
        wp, wn = C.POINTER(SpanTime)(), C.c_int(0)
        sp, sn = C.POINTER(SpanTime)(), C.c_int(0)
        _check(lib().ohw_engine_batch_times(self.h, int(i), C.byref(tp), C.byref(tn), C.byref(wp), C.byref(wn), C.byref(sp), C.byref(sn)))
        tb = self.batch_result(i)[0].encode("utf-8")
        return _token_times(tp, tn.value), _spans(wp, wn.value, tb), _spans(sp, sn.value, tb)

    def batch_confidence(self, i: int):
        """(token_probs, word_probs, segment_info) of recording i of the last batch call"""
        tp, tn = C.POINTER(TokenProb)(), C.c_int(0)
        wp, wn = C.POINTER(WordProb)(), C.c_int(0)
        sp, sn = C.POINTER(SegmentInfo)(), C.c_int(0)
        _check(lib().ohw_engine_batch_confidence(self.h, int(i), C.byref(tp), C.byref(tn), C.byref(wp), C.byref(wn), C.byref(sp), C.byref(sn)))
        tb = self.batch_result(i)[0].encode("utf-8")
        return _token_probs(tp, tn.value), _word_probs(wp, wn.value, tb), _segment_info(sp, sn.value)

    def score(self, audios: Sequence[AudioBuffer], texts_or_token_lists: Sequence) -> List[dict]:
        """ohw_engine_score_batch: how likely the unconstrained model finds the text the caller supplies for each recording (16 kHz,
        at most 30 s and n_text_ctx / 2 text tokens each).  An entry is a token-id list (the exact form) or a str / bytes, which
        goes through ohw_tokenize (not BPE merging: the caveat of set_commands).  -> per recording {"tokens": the last_token_probs
        dicts (logprob_decode NaN), "eot": the end-of-text row, "sum_logprob": the sum of logprob_all over both}.  N candidates
        for one recording: pass it N times"""
        if len(audios) != len(texts_or_token_lists):
            raise ValueError("score: one text or token list per recording")
        if not audios:
            return []
        if any(int(a.sample_rate) != 16000 for a in audios):
            raise ValueError("score: the recordings must be 16 kHz")
        lists = []
        for t in texts_or_token_lists:
            if isinstance(t, (str, bytes)):
                b = _text_bytes(t)
                out = np.zeros(max(len(b), 1), dtype=np.int32)
                n = lib().ohw_tokenize(self.ctx_h, b, _ip(out), int(out.size))
                if n < 0:
                    _raise(n)
                lists.append([int(x) for x in out[:n]])
            else:
                lists.append([int(x) for x in t])
        offs = np.zeros(len(lists) + 1, dtype=np.int32)
        offs[1:] = np.cumsum([len(t) for t in lists])
        toks = np.asarray([x for t in lists for x in t] or [0], dtype=np.int32)
        bufs = [np.ascontiguousarray(a.samples, dtype=np.float32) for a in audios]
        spans = (AudioSpan * len(bufs))()
        for i, b in enumerate(bufs):
            spans[i].samples = _fp(b) if b.size else C.cast(None, C.POINTER(C.c_float))
            spans[i].n = b.size
        res = (ScoreResultC * len(bufs))()
        _check(lib().ohw_engine_score_batch(self.h, spans, len(bufs), _ip(toks), _ip(offs), res))
        return [{"tokens": _token_probs(r.tokens, r.n_tokens), "eot": _token_probs(C.pointer(r.eot), 1)[0], "sum_logprob": float(r.sum_logprob_all)}
                for r in res]

    def set_detect_language(self, on: bool = True):
        """ohw_engine_set_detect_language: with language "auto" on a multilingual model, transcribe detects the language on its
        first window and transcribe_batch on every recording (default off: "auto" is "en", as in the reference)"""
        _check(lib().ohw_engine_set_detect_language(self.h, int(bool(on))))

    def last_language(self):
        """ohw_engine_last_language -> (id, code, probability) of the last transcribe (probability 1 when nothing was detected)"""
        i, pr = C.c_int32(0), C.c_float(0.0)
        _check(lib().ohw_engine_last_language(self.h, C.byref(i), C.byref(pr)))
        return int(i.value), lib().ohw_lang_id_to_code(i.value).decode(), float(pr.value)

    def _batch_call(self, what: str, audios: Sequence[AudioBuffer], languages: Optional[Sequence], call) -> List[TranscriptionResult]:
        """the shared body of transcribe_batch / transcribe_long_batch: language ids, audio spans, call(spans, langs or None, n,
        rate), then every recording's result and times"""
        langs = None
        if languages is not None:
            if len(languages) != len(audios):
                raise ValueError(f"{what}: one language per recording")
            ids = []
            for x in languages:
                if x is None or x == "auto":
                    ids.append(OHW_LANG_DETECT)
                elif isinstance(x, str):
                    i = int(lib().ohw_lang_code_to_id(x.encode()))
                    if i < 0:
                        raise ValueError(f"unknown language code {x!r}")
                    ids.append(i)
                else:
                    ids.append(int(x))
            langs = np.asarray(ids, dtype=np.int32)
        rates = {int(a.sample_rate) for a in audios}
        if len(rates) != 1:
            raise ValueError(f"{what}: the recordings must share one sample rate")
        bufs = [np.ascontiguousarray(a.samples, dtype=np.float32) for a in audios]
        spans = (AudioSpan * len(bufs))()
        for i, b in enumerate(bufs):
            spans[i].samples = _fp(b) if b.size else C.cast(None, C.POINTER(C.c_float))
            spans[i].n = b.size
        t0 = time.perf_counter()
        _check(call(spans, langs, len(bufs), rates.pop()))
        ms = int((time.perf_counter() - t0) * 1000)
        out = []
        for i in range(len(bufs)):
            r = self.batch_result(i)
            tt, words, segs = self.batch_times(i)
            out.append(TranscriptionResult(r[0], r[3], ms, tt, words, segs, *self.batch_confidence(i)))
        return out

    def transcribe_batch(self, audios: Sequence[AudioBuffer], languages: Optional[Sequence] = None) -> List[TranscriptionResult]:
        """ohw_engine_transcribe_batch: independent recordings of at most 30 s each in one call, batched longest first; results in
        submission order.  Tokens and quality of recording i: batch_result(i).  duration_ms is the whole call's.
        languages (ohw_engine_transcribe_batch_lang): one entry per recording - a language id, a code, or None / "auto" / -1 to
        detect that recording"""
        if not audios:
            return []

        def call(spans, langs, n, rate):
            if langs is None:
                return lib().ohw_engine_transcribe_batch(self.h, spans, n, rate)
            return lib().ohw_engine_transcribe_batch_lang(self.h, spans, _ip(langs), n, rate)
        return self._batch_call("transcribe_batch", audios, languages, call)

    def transcribe_long_batch(self, audios: Sequence[AudioBuffer], languages: Optional[Sequence] = None) -> List[TranscriptionResult]:
        """ohw_engine_transcribe_long_batch: independent recordings of any length in one call, each through the seek loop
        (OHW_WINDOW_SEEK, whatever set_window_mode says), one window of every live recording per decode batch.  Recording i's
        result equals transcribe() of it alone in the seek mode with batch invariance on.  Results in submission order; tokens,
        first window's quality and language: batch_result(i); every window's quality: long_batch_quality(i); times:
        batch_times(i).  languages as in transcribe_batch"""
        if not audios:
            return []

        def call(spans, langs, n, rate):
            return lib().ohw_engine_transcribe_long_batch(self.h, spans, _ip(langs) if langs is not None else None, n, rate)
        return self._batch_call("transcribe_long_batch", audios, languages, call)

    def set_vad(self, config: Optional[VadConfig] = None, detector: Optional[VadDetector] = None, plan: Optional[ChunkPlan] = None):
        """ohw_engine_set_vad: what transcribe_speech segments (config; its `enabled` is ignored), detects (detector) and chunks
        (plan) with; None = the defaults"""
        _check(lib().ohw_engine_set_vad(self.h, C.byref(config) if config is not None else None, C.byref(detector) if detector is not None else None,
                                        C.byref(plan) if plan is not None else None))

    def transcribe_speech(self, audios: Sequence[AudioBuffer], probs: Optional[Sequence] = None, languages: Optional[Sequence] = None) -> List[TranscriptionResult]:
        """ohw_engine_transcribe_speech: recordings of any length; the speech of each is found (the device detector, or
        probs[i] = (array, frame_samples) / None), cut at its pauses into chunks of at most 30 s, and the chunks of all recordings
        run as one transcribe_batch; times are on each recording's own clock.  Chunk c of recording i is transcribe_batch of its
        slice, bit for bit.  speech_chunks(i): the chunks and their quality records; languages as in transcribe_batch"""
        if not audios:
            return []
        fpr, keep = None, []
        if probs is not None:
            if len(probs) != len(audios):
                raise ValueError("transcribe_speech: one probs entry (or None) per recording")
            fpr = (FrameProbs * len(audios))()
            for i, pr in enumerate(probs):
                if pr is None:
                    fpr[i].p, fpr[i].n, fpr[i].frame_samples = C.cast(None, C.POINTER(C.c_float)), 0, 0
                else:
                    a = np.ascontiguousarray(pr[0], dtype=np.float32)
                    keep.append(a)
                    fpr[i].p, fpr[i].n, fpr[i].frame_samples = _fp(a) if a.size else C.cast(None, C.POINTER(C.c_float)), a.size, int(pr[1])

        def call(spans, langs, n, rate):
            return lib().ohw_engine_transcribe_speech_lang(self.h, spans, fpr, _ip(langs) if langs is not None else None, n, rate)
        return self._batch_call("transcribe_speech", audios, languages, call)

    def speech_chunks(self, i: int):
        """ohw_engine_speech_chunks: [{"start", "end" (samples), "first_segment", "n_segments", "quality": dict}] of recording i
        of the last transcribe_speech"""
        ch, n, q = C.POINTER(SpeechChunk)(), C.c_int(0), C.POINTER(WindowQuality)()
        _check(lib().ohw_engine_speech_chunks(self.h, int(i), C.byref(ch), C.byref(n), C.byref(q)))
        out = []
        for k in range(n.value):
            d = {name: getattr(q[k], name) for name, _ in WindowQuality._fields_}
            d["would_fallback"], d["no_speech"], d["failed"] = bool(d["would_fallback"]), bool(d["no_speech"]), bool(d["failed"])
            out.append({"start": int(ch[k].start), "end": int(ch[k].end), "first_segment": int(ch[k].first_segment),
                        "n_segments": int(ch[k].n_segments), "quality": d})
        return out

    def speech_segments(self, i: int):
        """ohw_engine_speech_segments: [(start, end, avg_probability)] of recording i of the last transcribe_speech"""
        sg, n = C.POINTER(SpeechSegment)(), C.c_int(0)
        _check(lib().ohw_engine_speech_segments(self.h, int(i), C.byref(sg), C.byref(n)))
        return [(int(sg[k].start), int(sg[k].end), float(sg[k].avg_probability)) for k in range(n.value)]

    def long_batch_quality(self, i: int):
        """one dict per window of recording i of the last transcribe_long_batch with every ohw_window_quality field"""
        q, n = C.POINTER(WindowQuality)(), C.c_int(0)
        _check(lib().ohw_engine_long_batch_quality(self.h, int(i), C.byref(q), C.byref(n)))
        out = []
        for k in range(n.value):
            d = {name: getattr(q[k], name) for name, _ in WindowQuality._fields_}
            d["would_fallback"], d["no_speech"], d["failed"] = bool(d["would_fallback"]), bool(d["no_speech"]), bool(d["failed"])
            out.append(d)
        return out

    def batch_result(self, i: int):
        """(text, tokens, quality dict, language) of recording i of the last transcribe_batch"""
        text, n = C.c_char_p(), C.c_size_t(0)
        toks, nt = C.POINTER(C.c_int32)(), C.c_int(0)
        q = C.POINTER(WindowQuality)()
        lang = C.create_string_buffer(8)
        _check(lib().ohw_engine_batch_result(self.h, int(i), C.byref(text), C.byref(n), C.byref(toks), C.byref(nt), C.byref(q), lang))
        d = {name: getattr(q[0], name) for name, _ in WindowQuality._fields_}
        d["would_fallback"], d["no_speech"], d["failed"] = bool(d["would_fallback"]), bool(d["no_speech"]), bool(d["failed"])
        return (C.string_at(text, n.value).decode("utf-8", "replace") if n.value else "", [int(toks[k]) for k in range(nt.value)], d,
                lang.value.decode())

    def last_quality(self):
        """[(n_tokens, avg_logprob, entropy, would_fallback)] per window of the last transcribe"""
        return [(q["n_tokens"], q["avg_logprob"], q["entropy"], q["would_fallback"]) for q in self.last_quality_ex()]

    def last_quality_ex(self):
        """one dict per window of the last transcribe with every ohw_window_quality field"""
        q = C.POINTER(WindowQuality)()
        n = C.c_int(0)
        _check(lib().ohw_engine_last_quality(self.h, C.byref(q), C.byref(n)))
        out = []
        for i in range(n.value):
            d = {name: getattr(q[i], name) for name, _ in WindowQuality._fields_}
            d["would_fallback"], d["no_speech"], d["failed"] = bool(d["would_fallback"]), bool(d["no_speech"]), bool(d["failed"])
            out.append(d)
        return out

    def set_decode_policy(self, temperature_inc: Optional[float] = None, entropy_thold: Optional[float] = None,
                          logprob_thold: Optional[float] = None, no_speech_thold: Optional[float] = None):
        """ohw_engine_set_decode_policy: whisper.cpp's defaults unless overridden; temperature_inc = 0 keeps every window at T = 0"""
        pol = DecodePolicy()
        lib().ohw_default_decode_policy(C.byref(pol))
        for k, v in (("temperature_inc", temperature_inc), ("entropy_thold", entropy_thold), ("logprob_thold", logprob_thold),
                     ("no_speech_thold", no_speech_thold)):
            if v is not None:
                setattr(pol, k, v)
        _check(lib().ohw_engine_set_decode_policy(self.h, C.byref(pol)))

    def set_fallback_on_device(self, on: bool = True):
        """ohw_engine_set_fallback_device: the temperature fallback samples on the device (default: on the host)"""
        _check(lib().ohw_engine_set_fallback_device(self.h, 1 if on else 0))

    def last_trace(self):
        """[(window, temperature, [sampled tokens, end-of-text included])] for every decode pass of the last transcribe"""
        p = C.POINTER(C.c_int32)()
        n = C.c_int(0)
        _check(lib().ohw_engine_last_trace(self.h, C.byref(p), C.byref(n)))
        out, i = [], 0
        while i + 3 <= n.value:
            w, t, k = p[i], p[i + 1], p[i + 2]
            out.append((int(w), t / 1000.0, [int(p[i + 3 + j]) for j in range(k)]))
            i += 3 + k
        return out

    def set_best_of(self, n: int):
        """ohw_engine_set_best_of: 1 (default) = one sampled sequence per rung above T = 0, 2..5 = that many candidates per pending
        window and rung, sampled on the device, the best kept (ohw_best_of_pick_host); a decode batch then holds
        max_batch // max(n, beam size, 1) windows"""
        _check(lib().ohw_engine_set_best_of(self.h, int(n)))

    def last_candidates(self):
        """[(window, temperature, kept j, [(tokens, logprobs) per candidate])] for every best-of rung of the last transcribe
        (ohw_engine_last_candidates / ohw_engine_last_candidate_logprobs); tokens are cut, end-of-text included when sampled"""
        p, n = C.POINTER(C.c_int32)(), C.c_int(0)
        q, m = C.POINTER(C.c_float)(), C.c_int(0)
        _check(lib().ohw_engine_last_candidates(self.h, C.byref(p), C.byref(n)))
        _check(lib().ohw_engine_last_candidate_logprobs(self.h, C.byref(q), C.byref(m)))
        out, i, f = [], 0, 0
        while i + 4 <= n.value:
            w, t, N, kept = p[i], p[i + 1], p[i + 2], p[i + 3]
            i += 4
            cands = []
            for _ in range(N):
                k = p[i]
                cands.append(([int(p[i + 1 + j]) for j in range(k)], np.array([q[f + j] for j in range(k)], dtype=np.float32)))
                i += 1 + k
                f += k
            out.append((int(w), t / 1000.0, int(kept), cands))
        assert f == m.value
        return out

    def set_beam_size(self, k: int):
        """ohw_engine_set_beam_size: 0 (default) = greedy at T = 0, 2..5 = beam search with k beams per window in every
        transcribe, transcribe_batch and transcribe_long_batch; a decode batch then holds max_batch // k windows"""
        _check(lib().ohw_engine_set_beam_size(self.h, int(k)))

    def set_force_len(self, n_tokens: int):
        """ohw_engine_set_force_len (measurement knob); refused while a beam size is set"""
        _check(lib().ohw_engine_set_force_len(self.h, int(n_tokens)))

    def set_window_mode(self, mode: int):
        """OHW_WINDOW_FIXED (0, default), OHW_WINDOW_SEEK (1, whisper.cpp's timestamp-driven loop) or OHW_WINDOW_FIXED_RECORDING_MEL
        (2: fixed cuts taken from the spectrogram of the whole recording)"""
        _check(lib().ohw_engine_set_window_mode(self.h, mode))

    def set_schedule(self, schedule: int, lanes: int = 0, merge: int = 0):
        """OHW_SCHEDULE_SEQUENTIAL / _PIPELINE / _LANES (default) for audio longer than max_batch windows"""
        _check(lib().ohw_engine_set_schedule(self.h, schedule, lanes, merge))

    def set_initial_prompt(self, prompt):
        """ohw_engine_set_initial_prompt / _tokens: text (str or bytes) or a list of token ids every window of every schedule is
        decoded behind (clipped to the last n_text_ctx / 2 - 1 tokens); "", None or [] clears it"""
        if prompt is None or isinstance(prompt, (str, bytes)):
            _check(lib().ohw_engine_set_initial_prompt(self.h, _text_bytes(prompt or "")))
        else:
            a = np.ascontiguousarray(list(prompt) or [0], dtype=np.int32)
            _check(lib().ohw_engine_set_initial_prompt_tokens(self.h, _ip(a), len(prompt)))

    def set_commands(self, phrases, penalty: float = COMMAND_PENALTY_DEFAULT):
        """ohw_engine_set_commands / _tokens: a closed list of phrases, strings (each tokenised as given and with a leading space,
        both forms under the string's index) or token-id lists (the exact form): every window is held to the list by `penalty`
        (State.set_command_table states the rule; float("inf") is the hard form); None or [] clears.  Holds for every state the
        engine decodes on; last_commands() tells which phrase each window was"""
        phrases = list(phrases or [])
        if _commands_are_text(phrases) or not phrases:
            _commands_text_call(lib().ohw_engine_set_commands, self.h, phrases, penalty)
        else:
            t, off, _ = _flat_phrases([list(p) for p in phrases], [0.0] * len(phrases))
            _check(lib().ohw_engine_set_commands_tokens(self.h, _ip(t), _ip(off), len(phrases), float(penalty)))

    def last_commands(self, recording: Optional[int] = None) -> List[dict]:
        """ohw_engine_last_commands (recording i of the last batch call: ohw_engine_batch_commands): per kept window
        {"window", "index", "list_logprob"}: index = the position in set_commands' list of the phrase the window's text tokens
        equal exactly, or -1; list_logprob = State.command_list_logprob's value of the kept pass; [] with no list set"""
        hits, n = C.POINTER(CommandHit)(), C.c_int()
        if recording is None:
            _check(lib().ohw_engine_last_commands(self.h, C.byref(hits), C.byref(n)))
        else:
            _check(lib().ohw_engine_batch_commands(self.h, int(recording), C.byref(hits), C.byref(n)))
        return [{"window": int(hits[i].window), "index": int(hits[i].phrase), "list_logprob": float(hits[i].list_logprob)} for i in range(n.value)]

    def set_repetition(self, penalty: float = 1.0, no_repeat_ngram_size: int = 0):
        """ohw_engine_set_repetition: faster-whisper's repetition_penalty and no_repeat_ngram_size on every state the engine decodes
        on (State.set_repeat_rule states the rule); the defaults turn both off"""
        _check(lib().ohw_engine_set_repetition(self.h, float(penalty), int(no_repeat_ngram_size)))

    def set_hot_phrases(self, phrases, boost=1.0):
        """ohw_engine_set_hot_phrases / _tokens: strings (each tokenised with and without a leading space) or token-id lists (the
        exact form) whose continuation is raised by `boost` logit units - one value, or one per phrase - while a row's own history
        ends in the front part of a phrase; None or [] clears.  Holds for every state the engine decodes on"""
        is_text, phrases, boosts = _hot_phrase_args(phrases, boost)
        if is_text or not phrases:
            _hot_phrase_text_call(lib().ohw_engine_set_hot_phrases, self.h, phrases, boosts)
        else:
            toks, off, b = _flat_phrases([list(p) for p in phrases], boosts)
            _check(lib().ohw_engine_set_hot_phrases_tokens(self.h, _ip(toks), _ip(off), _fp(b), len(phrases)))

    def set_prefill_chunk(self, positions: int):
        """ohw_engine_set_prefill_chunk: State.set_prefill_chunk on every state of the engine, those made later included"""
        _check(lib().ohw_engine_set_prefill_chunk(self.h, int(positions)))

    def set_carry_context(self, max_tokens: int = -1):
        """ohw_engine_set_carry_context: in the seek loops (OHW_WINDOW_SEEK transcribe, transcribe_long_batch) every window is
        decoded behind the tail of what the recording's earlier windows produced (whisper.cpp's default): -1 = up to the cap of
        n_text_ctx / 2 - 1 tokens, n > 0 = at most n (--max-context), 0 = off (the default here).  The initial prompt then only seeds
        the history.  No effect on fixed cuts and transcribe_batch, where every cut or recording is a call of its own"""
        _check(lib().ohw_engine_set_carry_context(self.h, int(max_tokens)))

    def set_stitch(self, overlap_s=5.0):
        """ohw_engine_set_stitch: the fixed cuts of transcribe (OHW_WINDOW_FIXED, OHW_WINDOW_FIXED_RECORDING_MEL; every schedule)
        overlap by overlap_s seconds (1 .. 15, a multiple of 20 ms) and neighbouring windows are merged where their text tokens
        agree (stitch_seams); None or 0 switches it off (the default).  No effect on OHW_WINDOW_SEEK, transcribe_batch,
        transcribe_long_batch, transcribe_speech or the pool"""
        ms = 0 if not overlap_s else int(round(float(overlap_s) * 1000.0))
        _check(lib().ohw_engine_set_stitch(self.h, ms))

    def stitch(self) -> float:
        """ohw_engine_stitch: the overlap in seconds, 0.0 = off"""
        return lib().ohw_engine_stitch(self.h) / 1000.0

    def last_seams(self) -> List[dict]:
        """ohw_engine_last_seams: one dict of SEAM_WORDS per seam of the last stitched transcribe (shift = matches = 0: unmatched,
        both windows kept whole)"""
        p, n = C.POINTER(C.c_int32)(), C.c_int(0)
        _check(lib().ohw_engine_last_seams(self.h, C.byref(p), C.byref(n)))
        return [{k: int(p[8 * i + j]) for j, k in enumerate(SEAM_WORDS) if k != "reserved"} for i in range(n.value)]

    def last_window_tokens(self) -> List[List[int]]:
        """ohw_engine_last_window_tokens: every window's kept tokens before the cut ([] when the last transcribe was not stitched)"""
        t, o, n = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)(), C.c_int(0)
        _check(lib().ohw_engine_last_window_tokens(self.h, C.byref(t), C.byref(o), C.byref(n)))
        return [[int(t[k]) for k in range(o[w], o[w + 1])] for w in range(n.value)]

    def _context(self, call) -> List[int]:
        p, n = C.POINTER(C.c_int32)(), C.c_int(0)
        _check(call(C.byref(p), C.byref(n)))
        return [int(p[k]) for k in range(n.value)]

    def last_contexts(self) -> List[List[int]]:
        """ohw_engine_last_context per window of the last transcribe: the context tokens ([prev] not included) its T = 0 pass was
        decoded behind; [] = none"""
        return [self._context(lambda p, n, w=w: lib().ohw_engine_last_context(self.h, w, p, n)) for w in range(len(self.last_quality_ex()))]

    def long_batch_contexts(self, i: int) -> List[List[int]]:
        """ohw_engine_long_batch_context per window of recording i of the last transcribe_long_batch"""
        return [self._context(lambda p, n, w=w: lib().ohw_engine_long_batch_context(self.h, int(i), w, p, n))
                for w in range(len(self.long_batch_quality(i)))]

    def set_audio_ctx(self, n):
        """ohw_engine_set_audio_ctx: 0 (default, off), a fixed context n, or "auto" (audio_ctx_for(len) for a recording of at most
        one window, full context beyond); a fixed context that does not cover a window's audio fails the transcribe"""
        _check(lib().ohw_engine_set_audio_ctx(self.h, _audio_ctx_arg(n)))

    def set_packed_encoder(self, on: bool = True):
        """ohw_engine_set_packed_encoder: State.set_packed_encoder on every state of the engine; under set_audio_ctx("auto")
        transcribe_batch then encodes a mixed batch at the sum of its contexts (same tokens, text and quality records)"""
        _check(lib().ohw_engine_set_packed_encoder(self.h, int(bool(on))))

    def last_tokens(self) -> List[int]:
        p = C.POINTER(C.c_int32)()
        n = C.c_int(0)
        lib().ohw_engine_last_tokens(self.h, C.byref(p), C.byref(n))
        return [int(p[i]) for i in range(n.value)]

    def benchmark(self, safety_margin: float) -> BenchmarkResult:
        a, b, c = C.c_float(0), C.c_float(0), C.c_float(0)
        _check(lib().ohw_engine_benchmark(self.h, safety_margin, C.byref(a), C.byref(b), C.byref(c)))
        return BenchmarkResult(a.value, b.value, c.value)

    def close(self):
        if getattr(self, "h", None):
            lib().ohw_engine_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class EnginePool(_ConfidenceMirror):
    """ohw_pool: one engine per device of one node behind the C ABI (the reference's `[gpu] devices` intent,
    src/config.rs:921-929).  transcribe() has WhisperEngine.transcribe's contract."""
    _WHO = "pool"

    def __init__(self, model_path: Optional[str], language: str = "auto", translate: bool = False, devices: Sequence[int] = (0,),
                 dtype: int = OHW_DTYPE_BF16, max_batch: int = 1, synthetic: Optional[Sequence[int]] = None, seed: int = 1234):
        """model_path: a ggml file; or synthetic = hparams list: procedural weights made on devices[0] (no file)"""
        ids = np.asarray(list(devices), dtype=np.int32)
        h = C.c_void_p()
        if synthetic is not None:
            hp = HParams(*[int(x) for x in synthetic])
            rc = lib().ohw_pool_create_synthetic(C.byref(hp), seed, language.encode(), int(translate), _ip(ids), len(ids), dtype, max_batch, C.byref(h))
        else:
            rc = lib().ohw_pool_create(str(model_path).encode(), language.encode(), int(translate), _ip(ids), len(ids), dtype, max_batch, C.byref(h))
        if rc != 0:
            _raise(rc)
        self.h = h

    def set_force_len(self, n_tokens: int):
        _check(lib().ohw_pool_set_force_len(self.h, n_tokens))

    def set_best_of(self, n: int):
        """ohw_pool_set_best_of: WhisperEngine.set_best_of(n) on every engine of the pool"""
        _check(lib().ohw_pool_set_best_of(self.h, int(n)))

    def set_beam_size(self, k: int):
        """ohw_pool_set_beam_size: WhisperEngine.set_beam_size(k) on every engine of the pool"""
        _check(lib().ohw_pool_set_beam_size(self.h, int(k)))

    def set_schedule(self, schedule: int, lanes: int = 0, merge: int = 0):
        _check(lib().ohw_pool_set_schedule(self.h, schedule, lanes, merge))

    @property
    def n_devices(self) -> int:
        return int(lib().ohw_pool_n_devices(self.h))

    @property
    def broadcast_kind(self) -> str:
        return lib().ohw_pool_broadcast_kind(self.h).decode()

    @property
    def broadcast_note(self) -> str:
        return lib().ohw_pool_broadcast_note(self.h).decode()

    def set_window_mode(self, mode: int):
        _check(lib().ohw_pool_set_window_mode(self.h, mode))

    def set_commands(self, phrases, penalty: float = COMMAND_PENALTY_DEFAULT):
        """ohw_pool_set_commands: WhisperEngine.set_commands (the text form) on every engine of the pool; None or [] clears"""
        phrases = list(phrases or [])
        if phrases and not _commands_are_text(phrases):
            raise ValueError("EnginePool.set_commands takes strings")
        _commands_text_call(lib().ohw_pool_set_commands, self.h, phrases, penalty)

    def set_repetition(self, penalty: float = 1.0, no_repeat_ngram_size: int = 0):
        """ohw_pool_set_repetition: WhisperEngine.set_repetition on every engine of the pool"""
        _check(lib().ohw_pool_set_repetition(self.h, float(penalty), int(no_repeat_ngram_size)))

    def set_hot_phrases(self, phrases, boost=1.0):
        """ohw_pool_set_hot_phrases: WhisperEngine.set_hot_phrases (the text form) on every engine of the pool; None or [] clears"""
        is_text, phrases, boosts = _hot_phrase_args(phrases, boost)
        if phrases and not is_text:
            raise ValueError("EnginePool.set_hot_phrases takes strings")
        _hot_phrase_text_call(lib().ohw_pool_set_hot_phrases, self.h, phrases, boosts)

    def set_initial_prompt(self, text):
        """ohw_pool_set_initial_prompt: WhisperEngine.set_initial_prompt(text) on every engine of the pool"""
        _check(lib().ohw_pool_set_initial_prompt(self.h, _text_bytes(text or "")))

    def set_carry_context(self, max_tokens: int = -1):
        """ohw_pool_set_carry_context: WhisperEngine.set_carry_context on every engine of the pool"""
        _check(lib().ohw_pool_set_carry_context(self.h, int(max_tokens)))

    def set_audio_ctx(self, n):
        """ohw_pool_set_audio_ctx: WhisperEngine.set_audio_ctx on every engine of the pool"""
        _check(lib().ohw_pool_set_audio_ctx(self.h, _audio_ctx_arg(n)))

    def set_packed_encoder(self, on: bool = True):
        """ohw_pool_set_packed_encoder: WhisperEngine.set_packed_encoder on every engine of the pool"""
        _check(lib().ohw_pool_set_packed_encoder(self.h, int(bool(on))))

    def set_detect_language(self, on: bool = True):
        """ohw_pool_set_detect_language: WhisperEngine.set_detect_language on every engine; the pool detects once, on its first"""
        _check(lib().ohw_pool_set_detect_language(self.h, int(bool(on))))

    def set_word_timestamps(self, heads: Optional[Sequence[Tuple[int, int]]]):
        """ohw_pool_set_word_timestamps: WhisperEngine.set_word_timestamps on every engine; None / empty = off"""
        hs = list(heads) if heads is not None else []
        arr = (AlignHead * len(hs))(*[AlignHead(int(l), int(h)) for l, h in hs]) if hs else None
        _check(lib().ohw_pool_set_word_timestamps(self.h, arr, len(hs)))

    def _last_text_bytes(self) -> bytes:
        full, n = C.c_char_p(), C.c_size_t(0)
        _check(lib().ohw_pool_last_text(self.h, C.byref(full), C.byref(n)))
        return C.string_at(full, n.value) if n.value else b""

    def last_token_times(self):
        """as WhisperEngine.last_token_times, gathered in recording order (window = the window of the recording)"""
        p, n = C.POINTER(TokenTime)(), C.c_int(0)
        _check(lib().ohw_pool_last_token_times(self.h, C.byref(p), C.byref(n)))
        return _token_times(p, n.value)

    def last_words(self):
        p, n = C.POINTER(SpanTime)(), C.c_int(0)
        _check(lib().ohw_pool_last_words(self.h, C.byref(p), C.byref(n)))
        return _spans(p, n.value, self._last_text_bytes())

    def last_segments(self):
        p, n = C.POINTER(SpanTime)(), C.c_int(0)
        _check(lib().ohw_pool_last_segments(self.h, C.byref(p), C.byref(n)))
        return _spans(p, n.value, self._last_text_bytes())

    def engine_handle(self, i: int):
        return lib().ohw_pool_engine(self.h, i)

    def set_decode_policy(self, **kw):
        pol = DecodePolicy()
        lib().ohw_default_decode_policy(C.byref(pol))
        for k, v in kw.items():
            setattr(pol, k, v)
        _check(lib().ohw_pool_set_decode_policy(self.h, C.byref(pol)))

    def set_fallback_on_device(self, on: bool = True):
        """ohw_pool_set_fallback_device: ohw_engine_set_fallback_device on every engine of the pool"""
        _check(lib().ohw_pool_set_fallback_device(self.h, 1 if on else 0))

    def transcribe(self, audio: AudioBuffer) -> TranscriptionResult:
        s = np.ascontiguousarray(audio.samples, dtype=np.float32)
        buf, lang, ms, info = C.create_string_buffer(256), C.create_string_buffer(8), C.c_uint64(0), AudioInfo()
        ptr = _fp(s) if s.size else C.cast(None, C.POINTER(C.c_float))
        rc = lib().ohw_pool_transcribe(self.h, ptr, s.size, audio.sample_rate, buf, len(buf), lang, C.byref(ms), C.byref(info))
        if rc != 0:
            _raise(rc, info)
        full, n = C.c_char_p(), C.c_size_t(0)
        _check(lib().ohw_pool_last_text(self.h, C.byref(full), C.byref(n)))
        text = C.string_at(full, n.value).decode("utf-8", "replace") if n.value else ""
        return TranscriptionResult(text, lang.value.decode(), int(ms.value))

    def last_tokens(self) -> List[int]:
        p, n = C.POINTER(C.c_int32)(), C.c_int(0)
        _check(lib().ohw_pool_last_tokens(self.h, C.byref(p), C.byref(n)))
        return [int(p[i]) for i in range(n.value)]

    def last_window_tokens(self) -> List[int]:
        q, n = C.POINTER(WindowQuality)(), C.c_int(0)
        _check(lib().ohw_pool_last_quality(self.h, C.byref(q), C.byref(n)))
        return [int(q[i].n_tokens) for i in range(n.value)]

    def close(self):
        if getattr(self, "h", None):
            lib().ohw_pool_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- model names: reference src/engine/whisper.rs:43-103 -----------------------------------------
_MODEL_FILES = {"tiny": "ggml-tiny.bin", "base": "ggml-base.bin", "small": "ggml-small.bin", "medium": "ggml-medium.bin",
                "large-v3": "ggml-large-v3.bin"}
_MODEL_ALIASES = {"large": "large-v3", "largev3": "large-v3"}


def model_filename(name: str) -> str:
    """WhisperModel::from_str + filename(): raises KeyError for names the reference rejects (e.g. 'tiny.en')"""
    key = name.lower()
    key = _MODEL_ALIASES.get(key, key)
    return _MODEL_FILES[key]


# approximate download sizes the reference shows to the user (src/engine/whisper.rs:82-92)
_MODEL_SIZES = {"tiny": 75_000_000, "base": 142_000_000, "small": 466_000_000, "medium": 1_500_000_000, "large-v3": 3_000_000_000}


def model_size_bytes(name: str) -> int:
    key = name.lower()
    return _MODEL_SIZES[_MODEL_ALIASES.get(key, key)]


_PRESET_MODEL = {"instant": "small", "balanced": "medium", "quality": "large-v3", "custom": "base"}


@dataclasses.dataclass
class TranscriptionConfig:
    """the fields of the reference's [transcription] table WhisperEngine::from_config reads (src/config.rs:662-696; defaults
    :641, :1080-1090)"""
    preset: str = "balanced"          # instant | balanced | quality | custom
    model: str = "large-v3"           # only used when preset == "custom"
    language: str = "auto"
    device: str = "cuda"
    translate: bool = False

    def effective_model(self) -> str:
        """src/config.rs:697-706 (known answers :1592-1622)"""
        return self.model if self.preset == "custom" else _PRESET_MODEL[self.preset]

    def engine_arguments(self, data_dir: Optional[str] = None):
        """(model_path, use_gpu) as from_config derives them"""
        import os
        try:
            fname = model_filename(self.effective_model())
        except KeyError:
            fname = model_filename("base")            # .parse().unwrap_or(WhisperModel::Base)
        if data_dir is None:
            data_dir = os.path.join(os.environ.get("XDG_DATA_HOME") or os.path.join(os.path.expanduser("~"), ".local", "share"), "openhush")
        return os.path.join(data_dir, "models", fname), self.device.lower() != "cpu"


def format_size(n: int) -> str:
    """reference src/engine/whisper.rs:444-458 (Rust {:.0} / {:.1} formatting: round half to even on the binary value)"""
    kb, mb, gb = 1024, 1024 ** 2, 1024 ** 3
    if n >= gb:
        return f"{n / gb:.1f} GB"
    if n >= mb:
        return f"{n / mb:.0f} MB"
    if n >= kb:
        return f"{n / kb:.0f} KB"
    return f"{n} B"


Pool = EnginePool
