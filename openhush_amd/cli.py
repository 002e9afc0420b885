"""`openhush transcribe FILE` plumbing over the MI355X engine (BASELINE.json config #1).

Mirrors the reference's one-shot CLI arm (reference src/main.rs:974-1077) and its WAV input contract
(reference src/input/audio.rs:348-434, `load_wav_file`): integer samples / 2^(bits-1), channel average, pad
with silence to 1.1 s; prints the same JSON fields as `--format json` (src/main.rs:1054-1066).
Any sample rate is accepted and resampled to 16 kHz (`--resampling-quality high` = the sinc resampler the reference's
default picks, `low` = linear: reference :394-407, config.audio.resampling_quality).

    python -m openhush_amd.cli transcribe audio.wav --model-path /path/ggml-small.bin [--format json]

Long recordings over several GPUs of one node (BASELINE.json config #4): launch the same command under
`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 -m openhush_amd.cli transcribe ...`;
the 30 s windows are dealt round-robin to the ranks (one GPU each), the token ids are gathered on rank 0 (RCCL), which
prints the result (openhush_amd/shard.py).
"""
from __future__ import annotations

import argparse
import json
import math
import os
import struct
import sys
import time

import numpy as np

SAMPLE_RATE = 16000
WHISPER_MIN_DURATION_SECS = 1.1   # reference src/input/audio.rs:34


def _read_riff(path: str):
    """(rate, channels, float32 interleaved samples) of a RIFF/WAVE file: PCM integers of 8 / 16 / 24 / 32 bits scaled by
    2^(bits-1) and 32-bit IEEE floats as they are - the two hound::SampleFormat arms of the reference (:369-382)"""
    with open(path, "rb") as f:
        blob = f.read()
    if len(blob) < 12 or blob[:4] != b"RIFF" or blob[8:12] != b"WAVE":
        raise ValueError(f"{path}: Failed to open WAV file: no RIFF/WAVE header")
    pos, fmt, data = 12, None, None
    while pos + 8 <= len(blob):
        cid, size = blob[pos:pos + 4], struct.unpack_from("<I", blob, pos + 4)[0]
        body = blob[pos + 8:pos + 8 + size]
        if cid == b"fmt " and len(body) >= 16:
            fmt = body
        elif cid == b"data":
            data = body                      # a truncated file keeps what is there (hound's filter_map(Result::ok))
            if fmt is not None:
                break
        pos += 8 + size + (size & 1)
    if fmt is None or data is None:
        raise ValueError(f"{path}: Failed to open WAV file: fmt or data chunk missing")
    tag, ch, rate, _, _, bits = struct.unpack_from("<HHIIHH", fmt, 0)
    if tag == 0xFFFE and len(fmt) >= 26:     # WAVE_FORMAT_EXTENSIBLE: the sub-format's first two bytes are the real tag
        tag = struct.unpack_from("<H", fmt, 24)[0]
    if ch < 1 or rate < 1:
        raise ValueError(f"{path}: Failed to open WAV file: bad channel count or rate")
    width = bits // 8
    data = data[:len(data) // width * width] if width else data
    if tag == 3 and bits == 32:
        s = np.frombuffer(data, "<f4").astype(np.float32)
    elif tag == 1 and width == 1:      # 8-bit WAV is unsigned; hound yields i8 = u8 - 128
        s = (np.frombuffer(data, np.uint8).astype(np.int32) - 128).astype(np.float32) / np.float32(1 << 7)
    elif tag == 1 and width == 2:
        s = np.frombuffer(data, "<i2").astype(np.float32) / np.float32(1 << 15)
    elif tag == 1 and width == 3:
        b = np.frombuffer(data, np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = np.where(v >= 1 << 23, v - (1 << 24), v)
        s = v.astype(np.float32) / np.float32(1 << 23)
    elif tag == 1 and width == 4:
        s = np.frombuffer(data, "<i4").astype(np.float32) / np.float32(2.0 ** 31)
    else:
        raise ValueError(f"{path}: unsupported WAV format (tag {tag}, {bits} bits)")
    return rate, ch, s


def load_wav_file(path: str, quality: str = "high") -> np.ndarray:
    """float32 mono 16 kHz samples like the reference's load_wav_file (src/input/audio.rs:348-434): any rate (resampled to
    16 kHz: `high` = the sinc resampler of :1007-1095, `low` = linear :972-990, as config.audio.resampling_quality picks -
    the reference's default is high), any of its sample formats, channels averaged, padded with silence to 1.1 s."""
    rate, ch, s = _read_riff(path)
    if ch > 1:   # average the channels (reference :384-391)
        s = (s[: len(s) // ch * ch].reshape(-1, ch).sum(axis=1, dtype=np.float32) / np.float32(ch)).astype(np.float32)
    if rate != SAMPLE_RATE:              # reference :394-407
        from . import engine as E
        s = E.resample_sinc(s, rate, SAMPLE_RATE) if quality == "high" else E.resample_linear(s, rate, SAMPLE_RATE)
    need = int(np.float32(SAMPLE_RATE) * np.float32(WHISPER_MIN_DURATION_SECS))
    if len(s) / SAMPLE_RATE < WHISPER_MIN_DURATION_SECS:
        s = np.concatenate([s, np.zeros(need - len(s), np.float32)])
    return np.ascontiguousarray(s, dtype=np.float32)


def _transcribe_ranks(args, audio, commands=()) -> int:
    """one process per GPU under torch.distributed.run: shard the windows, gather the tokens, rank 0 prints"""
    import torch
    import torch.distributed as dist
    from . import engine as E, shard
    rank, world, local = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), int(os.environ.get("LOCAL_RANK", "0"))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    torch.cuda.set_device(local)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
    E.validate_audio(audio.samples, audio.sample_rate)
    # rank 0 reads the file, the packed weights reach the other GPUs in one RCCL broadcast
    ctx = shard.load_model_broadcast(args.model_path, dist, world, rank, local, {"auto": E.OHW_DTYPE_AUTO, "bf16": E.OHW_DTYPE_BF16, "f16": E.OHW_DTYPE_F16}[args.dtype])
    p = ctx.default_params()
    if args.language != "auto":
        p.lang_id = E.lang_code_to_id(args.language)
    p.translate = 1 if args.translate else 0
    lang = "en" if args.language == "auto" else args.language
    if args.detect_language and args.language == "auto" and ctx.hp.n_vocab >= 51865:
        # every rank detects on window 0 of the recording: the same arithmetic on the same samples, so the same id everywhere
        st = E.State(ctx, 1)
        w0 = audio.samples[:E.CHUNK_SAMPLES]
        st.mel(w0[None, :], [len(w0)], E.OHW_MEL_ZERO_TAIL, want=False)
        st.encode(1)
        st.set_window_lang([E.OHW_LANG_DETECT])
        st.detect_window_lang(1)
        p.lang_id = int(st.window_lang(1)[0][0])
        st.close()
        lang = E.lang_id_to_code(p.lang_id)
    n_win = (len(audio.samples) + E.CHUNK_SAMPLES - 1) // E.CHUNK_SAMPLES
    t1 = time.perf_counter()
    by_index = args.mel == "recording"
    rep = _repetition(args)             # every rank decodes its windows under the same rule
    cmds = (commands, args.command_penalty) if commands else None        # and under the same list; the JSON carries no "commands" here
    runner = (shard.recording_window_runner(ctx, args.max_batch, audio.samples, p, repetition=rep, commands=cmds) if by_index
              else shard.engine_window_runner(ctx, args.max_batch, p, repetition=rep, commands=cmds))
    wins = shard.transcribe_sharded(runner, audio.samples, n_win, ctx.hp.n_text_ctx, dist, world, rank, torch.device("cuda", local),
                                    by_index=by_index)
    dt = time.perf_counter() - t1
    if rank == 0:
        text = b"".join(ctx.token_text(t) for w in wins for t in w if t < ctx.tok.eot).decode("utf-8", "replace").strip()
        name = args.model or args.model_path.rsplit("/", 1)[-1].replace("ggml-", "").rsplit(".", 1)[0]
        if args.format == "json":
            print(json.dumps({"text": text, "language": lang, "duration_ms": int(dt * 1e3), "audio_duration_secs": audio.duration_secs(),
                              "transcription_time_ms": int(dt * 1e3), "real_time_factor": dt / audio.duration_secs(),
                              "model": name.lower(), "gpus": world}, indent=2))
        else:
            print("\n--- Transcription ---")
            print(text)
            print("---")
            print(f"\nTime: {dt * 1e3:.0f}ms (RTF: {dt / audio.duration_secs():.3f}x) on {world} GPUs")
    dist.barrier()
    dist.destroy_process_group()
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="openhush_amd.cli")
    sub = ap.add_subparsers(dest="cmd", required=True)
    t = sub.add_parser("transcribe")
    t.add_argument("file")
    many = sub.add_parser("transcribe-many", help="several recordings of any length in one call, each through whisper.cpp's seek loop, one "
                                                  "window of every recording per decode batch; prints one JSON object per line, in argument order")
    many.add_argument("files", nargs="+", metavar="FILE")
    many.add_argument("--carry-context", action="store_true",
                      help="decode every window behind the text of the recording's earlier windows (whisper.cpp's default; off by default "
                           "here); --prompt then only seeds that history.  The contexts are not part of the JSON")
    many.add_argument("--max-context", type=_max_context_arg, default=-1, metavar="N",
                      help="with --carry-context: at most N tokens of earlier text (whisper.cpp's --max-context); -1 (default): up to half "
                           "the model's text context")
    for sp_ in (t, many):
        _add_transcribe_options(sp_)
    args = ap.parse_args(argv)
    if args.cmd == "transcribe-many":
        return _transcribe_many(args)
    return _transcribe_one(args)


def _read_commands(args):
    """--commands FILE -> the phrases, () without the option, None after an error message"""
    if not args.commands:
        return ()
    from . import engine as E
    try:
        with open(args.commands, encoding="utf-8") as f:
            phrases = E.parse_commands(f.read())
        if not phrases:
            raise ValueError("the file holds no phrase")
        if len(phrases) > E.PHRASE_MAX_PHRASES // 2:
            raise ValueError(f"{len(phrases)} phrases, at most {E.PHRASE_MAX_PHRASES // 2} fit (each in two forms)")
        return phrases
    except (OSError, ValueError) as ex:
        print(f"error: --commands: {ex}", file=sys.stderr)
        return None


def _commands_json(hits, phrases):
    """WhisperEngine.last_commands() as the JSON carries it: the phrase's text beside its index, null for a list_logprob that is not finite"""
    return [{"window": h["window"], "index": h["index"], "phrase": phrases[h["index"]] if h["index"] >= 0 else None,
             "list_logprob": h["list_logprob"] if math.isfinite(h["list_logprob"]) else None} for h in hits]


def _read_hot_phrases(args):
    """--hot-phrases FILE with --hot-phrase-boost X -> (phrases, boosts), () without the option, None after an error message"""
    if not args.hot_phrases:
        return ()
    from . import engine as E
    try:
        with open(args.hot_phrases, encoding="utf-8") as f:
            return E.parse_hot_phrases(f.read(), args.hot_phrase_boost)
    except (OSError, ValueError) as ex:
        print(f"error: --hot-phrases: {ex}", file=sys.stderr)
        return None


def _add_transcribe_options(t):
    t.add_argument("--model-path", required=True, help="ggml-*.bin model file")
    t.add_argument("--model", default=None, help="name printed in the JSON (default: derived from the file name)")
    t.add_argument("--language", default="auto")
    t.add_argument("--translate", action="store_true")
    t.add_argument("--format", default="text", choices=["text", "json"])
    t.add_argument("--device", default="hip:0")
    t.add_argument("--dtype", default="auto", choices=["auto", "bf16", "f16"],
                   help="auto (default): the model file's own precision - f16 for the stock ggml files (ftype 1), whose weights then stay exact")
    t.add_argument("--max-batch", type=int, default=8)
    t.add_argument("--resampling-quality", default="high", choices=["low", "high"],
                   help="for files that are not 16 kHz (the reference's config.audio.resampling_quality, default high = sinc)")
    t.add_argument("--mel", default="window", choices=["window", "recording"],
                   help="window (default): every 30 s cut is its own call; recording: the cuts are taken from the spectrogram of the whole "
                        "recording (one clamp maximum, real samples across the 30 s marks), as whisper.cpp computes it for one call")
    t.add_argument("--audio-ctx", default="0", metavar="N|auto",
                   help="reduced audio context (whisper.cpp's audio_ctx): 0 (default) the full 30 s context; N encoder positions per window "
                        "(320 samples each; audio past them is an error, never dropped); auto: sized to a recording of at most 30 s")
    t.add_argument("--prompt", default="", metavar="TEXT",
                   help="initial prompt (whisper.cpp's initial_prompt): names, jargon and spelling hints every window is decoded behind")
    t.add_argument("--hot-phrases", default=None, metavar="FILE",
                   help="hot phrases (names, product terms): one phrase per line, optionally a tab and its boost in logit units. While a "
                        "window's own tokens end in the front part of a phrase, its next token is raised by the boost")
    t.add_argument("--hot-phrase-boost", type=float, default=2.0, metavar="X",
                   help="the boost of every --hot-phrases line that carries none (default 2.0)")
    t.add_argument("--commands", default=None, metavar="FILE",
                   help="a closed list of phrases, one per line: every window is held to the list (whisper.cpp's grammar for a fixed "
                        "vocabulary) and the JSON gains \"commands\": per window the index and text of the phrase it was, or -1, and "
                        "list_logprob, the log-probability that the unconstrained model starts a listed phrase")
    t.add_argument("--command-penalty", type=_command_penalty_arg, default=100.0, metavar="X|inf",
                   help="how far a text token that leaves the list, and end-of-text inside a phrase, is lowered, in logit units: "
                        "0 < X <= 1000, or inf for a hard list (default 100, whisper.cpp's grammar_penalty)")
    t.add_argument("--repetition-penalty", type=_repetition_penalty_arg, default=1.0, metavar="X",
                   help="scale the logit of every text token a window has already emitted away from the sampler (x / X above 0, "
                        "x * X below; faster-whisper's repetition_penalty), 0.01..100; 1.0 (default): off")
    t.add_argument("--no-repeat-ngram-size", type=_no_repeat_ngram_arg, default=0, metavar="N",
                   help="never emit a text token that would complete an N-gram the window already holds (faster-whisper's "
                        "no_repeat_ngram_size), 0..32; 0 (default): off")
    t.add_argument("--packed-encoder", action="store_true",
                   help="run the encoder on the sum of the windows' contexts when a batch carries per-window contexts (the engine's "
                        "transcribe_batch under --audio-ctx auto); same output, default off")
    t.add_argument("--detect-language", action="store_true",
                   help="with --language auto on a multilingual model: detect the language on the first 30 s window and decode in it "
                        "(default: auto means en, as in the reference); the JSON language field carries the detected code")
    t.add_argument("--beam-size", type=_beam_size_arg, default=0, metavar="K",
                   help="beam search with K beams (2..5) as the temperature-0 strategy (whisper.cpp's beam_size); 0 (default): greedy. "
                        "A decode batch then holds max-batch / K windows; the fallback temperatures sample as before")
    t.add_argument("--best-of", type=_best_of_arg, default=1, metavar="N",
                   help="candidates per window (1..5) on every fallback temperature above 0 (whisper.cpp's best_of), sampled on the "
                        "device, the best kept; 1 (default): one sampled sequence. A decode batch then holds max-batch / max(N, K) windows")
    t.add_argument("--word-timestamps", action="store_true",
                   help="align every window's tokens on the device and add \"segments\" and \"words\" arrays (text, t0, t1 in seconds) to "
                        "the JSON; needs --align-heads")
    t.add_argument("--confidence", action="store_true",
                   help="score every window's kept tokens with the unconstrained model on the device (a teacher-forced pass, openai-"
                        "whisper's word probability) and add to the JSON: \"probability\" on each word (a top-level \"word_probs\" "
                        "without --word-timestamps), \"avg_logprob\" and \"no_speech_prob\" on segments, and \"tokens_conf\" per text token")
    t.add_argument("--stitch", action="store_true",
                   help="overlap the 30 s cuts of a long recording and merge neighbouring windows where their tokens agree, so that a "
                        "word on a cut is heard whole by one of them; the JSON gains \"seams\": per seam its left window, its time on "
                        "the recording's clock, and the shift and matches of the merge (0 and 0: no agreement, both windows kept whole)")
    t.add_argument("--stitch-overlap", type=float, default=None, metavar="S",
                   help="with --stitch: seconds of audio neighbouring windows share, 1..15 in steps of 0.02 (default 5)")
    _add_vad_options(t)
    t.add_argument("--align-heads", default="", metavar="L.H,L.H,...",
                   help="the (decoder layer, head) pairs whose cross-attention carries the alignment, at most 32; no preset ships "
                        "(INTEGRATION.md says where upstream lists them per checkpoint)")


def _confidence_json(doc: dict, with_times: bool, segments, token_probs, word_probs, segment_info):
    """--confidence: the fields the option adds to one recording's JSON document"""
    if not with_times:
        doc["segments"] = [{"text": s["text"], "t0": s["t0"], "t1": s["t1"]} for s in segments]
        doc["word_probs"] = [{"text": w["text"], "probability": w["probability"]} for w in word_probs]
    else:
        for w, p in zip(doc["words"], word_probs):
            w["probability"] = p["probability"]
    for s, info in zip(doc["segments"], segment_info):
        s["avg_logprob"] = None if info["avg_logprob"] != info["avg_logprob"] else info["avg_logprob"]      # NaN: the window was not scored
        s["no_speech_prob"] = info["no_speech_prob"]
    doc["tokens_conf"] = token_probs


def _stitch_ms(args, E):
    """--stitch [--stitch-overlap S] -> the overlap in ms, 0 without --stitch, None after an error message"""
    if not args.stitch:
        if args.stitch_overlap is not None:
            print("error: --stitch-overlap sets the overlap of --stitch; it needs --stitch", file=sys.stderr)
            return None
        return 0
    s = 5.0 if args.stitch_overlap is None else args.stitch_overlap
    ms = int(round(s * 1000.0)) if math.isfinite(s) else -1
    try:
        if ms == 0 or abs(ms - s * 1000.0) > 1e-6:
            raise ValueError
        E.stitch_plan_host(0, ms)
    except (ValueError, E.WhisperError):
        print(f"error: --stitch-overlap takes 1..15 seconds in steps of 0.02, not '{args.stitch_overlap}'", file=sys.stderr)
        return None
    return ms


def _seams_json(seams, stitch_ms: int, duration: float):
    """--stitch: per seam its left window, the seam time (the middle of the audio the two windows share) and the merge's words"""
    hop = 30.0 - stitch_ms / 1000.0
    return [{"window": s["left_window"], "time": ((s["left_window"] + 1) * hop + min(duration, s["left_window"] * hop + 30.0)) / 2.0,
             "shift": s["shift"], "matches": s["matches"]} for s in seams]


def _add_vad_options(t):
    t.add_argument("--vad", action="store_true",
                   help="speech-aware windows: find the speech on the device (a model-free spectral detector, not Silero), cut at the "
                        "pauses into chunks of at most 30 s and run the chunks as one batch (WhisperEngine.transcribe_speech); "
                        "JSON output gains \"chunks\"")
    t.add_argument("--vad-threshold", type=float, default=None, metavar="X", help="speech probability that opens a segment (default 0.5)")
    t.add_argument("--vad-min-silence-ms", type=int, default=None, metavar="N", help="pause that ends a segment (default 700)")
    t.add_argument("--vad-max-gap-ms", type=int, default=None, metavar="N", help="largest pause inside one chunk (default 2000)")


def _vad_settings(args, E):
    """-> (VadConfig, ChunkPlan) for --vad, or None after printing an error"""
    if not args.vad:
        if args.vad_threshold is not None or args.vad_min_silence_ms is not None or args.vad_max_gap_ms is not None:
            print("error: --vad-threshold, --vad-min-silence-ms and --vad-max-gap-ms need --vad", file=sys.stderr)
            return None
        return ()
    cfg, plan = E.default_vad_config(), E.default_chunk_plan()
    if args.vad_threshold is not None:
        if not 0.0 < args.vad_threshold < 1.0:
            print("error: --vad-threshold must be between 0 and 1", file=sys.stderr)
            return None
        cfg.threshold = args.vad_threshold
    if args.vad_min_silence_ms is not None:
        if args.vad_min_silence_ms < 0:
            print("error: --vad-min-silence-ms must not be negative", file=sys.stderr)
            return None
        cfg.min_silence_ms = args.vad_min_silence_ms
    if args.vad_max_gap_ms is not None:
        if args.vad_max_gap_ms < 0:
            print("error: --vad-max-gap-ms must not be negative", file=sys.stderr)
            return None
        plan.max_gap_ms = args.vad_max_gap_ms
    return cfg, plan


def _chunks_json(eng, i):
    return [{"start": c["start"] / SAMPLE_RATE, "end": c["end"] / SAMPLE_RATE} for c in eng.speech_chunks(i)]


def _beam_size_arg(v: str) -> int:
    try:
        k = int(v)
    except ValueError:
        k = -1
    if k != 0 and not 2 <= k <= 5:
        raise argparse.ArgumentTypeError(f"takes 0 (greedy) or a beam size in 2..5, not '{v}'")
    return k


def _repetition_penalty_arg(v: str) -> float:
    try:
        x = float(v)
    except ValueError:
        x = float("nan")
    if not 0.01 <= x <= 100.0:                      # false for NaN
        raise argparse.ArgumentTypeError(f"takes a penalty in 0.01..100 (1.0: off), not '{v}'")
    return x


def _command_penalty_arg(v: str) -> float:
    x = float("nan")
    try:
        x = float(v)
    except ValueError:
        pass
    if not (0.0 < x <= 1000.0 or x == float("inf")):          # false for NaN
        raise argparse.ArgumentTypeError(f"takes a penalty in (0, 1000] or inf, not '{v}'")
    return x


def _no_repeat_ngram_arg(v: str) -> int:
    try:
        n = int(v)
    except ValueError:
        n = -1
    if not 0 <= n <= 32:
        raise argparse.ArgumentTypeError(f"takes an n-gram size in 0..32 (0: off), not '{v}'")
    return n


def _repetition(args):
    """(--repetition-penalty, --no-repeat-ngram-size) when either is on, None when both are off"""
    return (args.repetition_penalty, args.no_repeat_ngram_size) if args.repetition_penalty != 1.0 or args.no_repeat_ngram_size != 0 else None


def _best_of_arg(v: str) -> int:
    try:
        n = int(v)
    except ValueError:
        n = -1
    if not 1 <= n <= 5:
        raise argparse.ArgumentTypeError(f"takes a number of candidates in 1..5, not '{v}'")
    return n


def _max_context_arg(v: str) -> int:
    try:
        n = int(v)
    except ValueError:
        n = -2
    if n < -1:
        raise argparse.ArgumentTypeError(f"takes -1 (the model's cap) or a token count, not '{v}'")
    return n


def _check_beam(args) -> bool:
    """--beam-size and --best-of against the other options, before any model is loaded"""
    if args.best_of > 1:
        if args.best_of > args.max_batch:
            print(f"error: --best-of {args.best_of} needs --max-batch >= {args.best_of} (a window takes one decoder row per candidate)", file=sys.stderr)
            return False
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            print("error: --best-of is not supported under torch.distributed.run (one process per GPU)", file=sys.stderr)
            return False
    if args.beam_size == 0:
        return True
    if args.beam_size > args.max_batch:
        print(f"error: --beam-size {args.beam_size} needs --max-batch >= {args.beam_size} (a window takes one decoder row per beam)", file=sys.stderr)
        return False
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        print("error: --beam-size is not supported under torch.distributed.run (one process per GPU)", file=sys.stderr)
        return False
    return True


def _align_heads(args):
    """the --align-heads pairs when --word-timestamps is on ([] when off); None after printing an error"""
    if not args.word_timestamps:
        return []
    try:
        align_heads = [(int(x.split(".")[0]), int(x.split(".")[1])) for x in args.align_heads.split(",") if x.strip()]
    except (ValueError, IndexError):
        align_heads = []
    if not align_heads:
        print("error: --word-timestamps needs --align-heads L.H,L.H,... (decoder layer . head)", file=sys.stderr)
        return None
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        print("error: --word-timestamps is not supported under torch.distributed.run (one process per GPU)", file=sys.stderr)
        return None
    return align_heads


def _transcribe_many(args) -> int:
    """`transcribe-many FILE [FILE ...]`: WhisperEngine.transcribe_long_batch over the files; one JSON object per line with the
    fields of `transcribe --format json`.  The times are the whole call's: transcription_time_ms and duration_ms are the same in
    every line, real_time_factor is that time over the summed duration of all files."""
    align_heads = _align_heads(args)
    if align_heads is None or not _check_beam(args):
        return 1
    if args.max_context != -1 and not args.carry_context:
        print("error: --max-context limits the carried context; it needs --carry-context", file=sys.stderr)
        return 1
    if args.stitch or args.stitch_overlap is not None:
        print("error: --stitch merges the fixed cuts of `transcribe`; transcribe-many runs the seek loop, which has no cuts", file=sys.stderr)
        return 1
    from . import engine as E
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        print("error: transcribe-many is not supported under torch.distributed.run (one process per GPU)", file=sys.stderr)
        return 1
    vad = _vad_settings(args, E)
    if vad is None:
        return 1
    if vad and args.carry_context:
        print("error: --vad decodes the chunks in parallel; --carry-context has no effect there", file=sys.stderr)
        return 1
    try:
        audio_ctx = E._audio_ctx_arg(args.audio_ctx)
        if audio_ctx != 0 and not vad:
            raise ValueError
    except ValueError:
        print("error: transcribe-many runs every window at the full audio context; --audio-ctx applies only with --vad", file=sys.stderr)
        return 1
    hot = _read_hot_phrases(args)
    if hot is None:
        return 1
    commands = _read_commands(args)
    if commands is None:
        return 1
    audios = []
    for f in args.files:
        if not os.path.isfile(f):
            print(f"error: File not found: {f}", file=sys.stderr)
            return 1
        try:
            audios.append(E.AudioBuffer(load_wav_file(f, args.resampling_quality), SAMPLE_RATE))
        except (ValueError, struct.error, EOFError) as ex:
            print(f"error: {ex}", file=sys.stderr)
            return 1
    use_gpu = args.device.lower() != "cpu"
    dev = int(args.device.split(":")[1]) if ":" in args.device else 0
    t0 = time.perf_counter()
    eng = E.WhisperEngine.new(args.model_path, args.language, args.translate, use_gpu, dev,
                              {"auto": E.OHW_DTYPE_AUTO, "bf16": E.OHW_DTYPE_BF16, "f16": E.OHW_DTYPE_F16}[args.dtype], args.max_batch)
    print(f"Model loaded in {1e3 * (time.perf_counter() - t0):.0f}ms", file=sys.stderr)
    if args.prompt:
        eng.set_initial_prompt(args.prompt)
    if hot:
        eng.set_hot_phrases(*hot)
    if _repetition(args):
        eng.set_repetition(*_repetition(args))
    if commands:
        try:
            eng.set_commands(commands, args.command_penalty)
        except E.WhisperError as ex:
            print(f"error: --commands: {ex}", file=sys.stderr)
            return 1
    if args.beam_size:
        eng.set_beam_size(args.beam_size)
    if args.best_of > 1:
        eng.set_best_of(args.best_of)
    if args.carry_context and args.max_context != 0:      # --max-context 0 carries nothing, as in whisper.cpp
        eng.set_carry_context(args.max_context)
    if args.packed_encoder:
        eng.set_packed_encoder(True)
    if args.detect_language:
        eng.set_detect_language(True)
    if align_heads:
        try:
            eng.set_word_timestamps(align_heads)
        except E.WhisperError as ex:
            print(f"error: {ex}", file=sys.stderr)
            return 1
    if args.confidence:
        eng.set_confidence(True)
    t1 = time.perf_counter()
    try:
        if vad:
            eng.set_vad(vad[0], None, vad[1])
            if audio_ctx != 0:
                eng.set_audio_ctx(audio_ctx)
            results = eng.transcribe_speech(audios)
        else:
            results = eng.transcribe_long_batch(audios)
    except E.WhisperError as ex:
        print(f"error: {ex}", file=sys.stderr)
        return 1
    dt = time.perf_counter() - t1
    total = sum(a.duration_secs() for a in audios)
    name = args.model or args.model_path.rsplit("/", 1)[-1].replace("ggml-", "").rsplit(".", 1)[0]
    for i, (a, res) in enumerate(zip(audios, results)):
        doc = {"text": res.text, "language": res.language, "duration_ms": res.duration_ms,
               "audio_duration_secs": a.duration_secs(), "transcription_time_ms": int(dt * 1e3),
               "real_time_factor": dt / total, "model": name.lower()}
        if vad:
            doc["chunks"] = _chunks_json(eng, i)
        if commands:
            doc["commands"] = _commands_json(eng.last_commands(i), commands)
        if align_heads:
            doc["segments"] = [{"text": s["text"], "t0": s["t0"], "t1": s["t1"]} for s in res.segments]
            doc["words"] = [{"text": w["text"], "t0": w["t0"], "t1": w["t1"]} for w in res.words]
        if args.confidence:
            _confidence_json(doc, bool(align_heads), res.segments, res.token_probs, res.word_probs, res.segment_info)
        print(json.dumps(doc))
    eng.close()
    return 0


def _transcribe_one(args) -> int:
    align_heads = _align_heads(args)
    if align_heads is None or not _check_beam(args):
        return 1

    from . import engine as E
    try:
        audio_ctx = E._audio_ctx_arg(args.audio_ctx)
    except ValueError:
        print(f"error: --audio-ctx takes 0, a positive number or 'auto', not '{args.audio_ctx}'", file=sys.stderr)
        return 1
    stitch_ms = _stitch_ms(args, E)
    if stitch_ms is None:
        return 1
    hot = _read_hot_phrases(args)
    if hot is None:
        return 1
    commands = _read_commands(args)
    if commands is None:
        return 1
    if not os.path.isfile(args.file):            # reference src/main.rs:985-987 and tests/cli_integration.rs:262-269
        print(f"error: File not found: {args.file}", file=sys.stderr)
        return 1
    try:
        audio = E.AudioBuffer(load_wav_file(args.file, args.resampling_quality), SAMPLE_RATE)
    except (ValueError, struct.error, EOFError) as ex:
        print(f"error: {ex}", file=sys.stderr)
        return 1
    vad = _vad_settings(args, E)
    if vad is None:
        return 1
    if vad and args.mel == "recording":
        print("error: --vad cuts chunks as fixed windows of their own; --mel recording does not apply", file=sys.stderr)
        return 1
    if stitch_ms and (vad or int(os.environ.get("WORLD_SIZE", "1")) > 1):
        print("error: --stitch merges the fixed cuts of one engine; it does not apply to --vad or under torch.distributed.run", file=sys.stderr)
        return 1
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        if vad:
            print("error: --vad is not supported under torch.distributed.run (one process per GPU)", file=sys.stderr)
            return 1
        if audio_ctx != 0:
            print("error: --audio-ctx is not supported under torch.distributed.run (one process per GPU)", file=sys.stderr)
            return 1
        if args.prompt:
            print("error: --prompt is not supported under torch.distributed.run (one process per GPU)", file=sys.stderr)
            return 1
        if hot:
            print("error: --hot-phrases is not supported under torch.distributed.run (one process per GPU)", file=sys.stderr)
            return 1
        if args.confidence:
            print("error: --confidence is not supported under torch.distributed.run (one process per GPU)", file=sys.stderr)
            return 1
        return _transcribe_ranks(args, audio, commands)
    use_gpu = args.device.lower() != "cpu"                    # reference src/main.rs:1037
    dev = int(args.device.split(":")[1]) if ":" in args.device else 0
    t0 = time.perf_counter()
    eng = E.WhisperEngine.new(args.model_path, args.language, args.translate, use_gpu, dev,
                              {"auto": E.OHW_DTYPE_AUTO, "bf16": E.OHW_DTYPE_BF16, "f16": E.OHW_DTYPE_F16}[args.dtype], args.max_batch)
    print(f"Model loaded in {1e3 * (time.perf_counter() - t0):.0f}ms", file=sys.stderr)
    if args.mel == "recording":
        eng.set_window_mode(E.OHW_WINDOW_FIXED_RECORDING_MEL)
    if audio_ctx != 0:
        eng.set_audio_ctx(audio_ctx)
    if args.prompt:
        eng.set_initial_prompt(args.prompt)
    if hot:
        eng.set_hot_phrases(*hot)
    if _repetition(args):
        eng.set_repetition(*_repetition(args))
    if commands:
        try:
            eng.set_commands(commands, args.command_penalty)
        except E.WhisperError as ex:
            print(f"error: --commands: {ex}", file=sys.stderr)
            return 1
    if args.beam_size:
        eng.set_beam_size(args.beam_size)
    if args.best_of > 1:
        eng.set_best_of(args.best_of)
    if args.packed_encoder:
        eng.set_packed_encoder(True)
    if args.detect_language:
        eng.set_detect_language(True)
    if align_heads:
        try:
            eng.set_word_timestamps(align_heads)
        except E.WhisperError as ex:
            print(f"error: {ex}", file=sys.stderr)
            return 1
    if args.confidence:
        eng.set_confidence(True)
    if stitch_ms:
        eng.set_stitch(stitch_ms / 1000.0)
    t1 = time.perf_counter()
    if vad:
        try:
            eng.set_vad(vad[0], None, vad[1])
            res = eng.transcribe_speech([audio])[0]
        except E.WhisperError as ex:
            print(f"error: {ex}", file=sys.stderr)
            return 1
    else:
        res = eng.transcribe(audio)
    dt = time.perf_counter() - t1
    rtf = dt / audio.duration_secs()
    name = args.model or args.model_path.rsplit("/", 1)[-1].replace("ggml-", "").rsplit(".", 1)[0]
    if args.format == "json":
        doc = {"text": res.text, "language": res.language, "duration_ms": res.duration_ms,
               "audio_duration_secs": audio.duration_secs(), "transcription_time_ms": int(dt * 1e3),
               "real_time_factor": rtf, "model": name.lower()}
        if vad:
            doc["chunks"] = _chunks_json(eng, 0)
        if commands:
            doc["commands"] = _commands_json(eng.last_commands(0 if vad else None), commands)
        if align_heads:
            doc["segments"] = [{"text": s["text"], "t0": s["t0"], "t1": s["t1"]} for s in (res.segments if vad else eng.last_segments())]
            doc["words"] = [{"text": w["text"], "t0": w["t0"], "t1": w["t1"]} for w in (res.words if vad else eng.last_words())]
        if stitch_ms:
            doc["seams"] = _seams_json(eng.last_seams(), stitch_ms, audio.duration_secs())
        if args.confidence:
            if vad:
                _confidence_json(doc, bool(align_heads), res.segments, res.token_probs, res.word_probs, res.segment_info)
            else:
                _confidence_json(doc, bool(align_heads), eng.last_segments(), eng.last_token_probs(), eng.last_word_probs(), eng.last_segment_info())
        print(json.dumps(doc, indent=2))
    else:
        print("\n--- Transcription ---")
        print(res.text)
        print("---")
        print(f"\nTime: {dt * 1e3:.0f}ms (RTF: {rtf:.3f}x)")
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
