"""Config #5 on one MI355X: large-v3, streaming chunks, beam = 5 (two alternating hipGraph-captured decoder steps), energy VAD
in front (the reference's RNNoise and Silero models are not available offline).  A chunk timer of --chunk
seconds over a synthetic recording; prints the per-chunk latency of StreamingSession.transcribe_job (mel + encoder +
cross-K/V + beam search of --tokens forced steps, detokenise) and the real-time factor of the stream.

    python tools/streaming_latency.py [--chunk 5 --chunks 12 --beam 5 --tokens 48]

--audio-ctx N|auto runs the chunks under a reduced audio context (StreamingSession(audio_ctx=...)); every run also reports the
state's own device times per chunk (encode_ms, decode ms per step).  --batch B leaves the session aside and takes B windows of
--chunk seconds through mel -> encode -> greedy (--tokens forced steps) as ONE batch, --reps times: the server-shaped case.
--mixed LO:HI (with --batch B): the B chunk lengths are drawn from a seeded uniform range of LO .. HI seconds (--seed) and the
batch runs three legs, one JSON line each: `ragged` (State.set_window_ctx: every window at audio_ctx_for of its own length
inside the largest of them), `envelope` (uniform at that largest context) and `off` (the full context); --legs picks a subset
and also takes `packed`: the `ragged` leg with State.set_packed_encoder(True), the encoder on sum(n_ctx) rows ("enc_rows").
--with-long K makes the first K windows of the mix 30 s long (a batch of short chunks behind one long recording).
LO = HI = 30 is the uniform mix at which `ragged` must not lose to `envelope`.
--hot-phrases N (with --batch B, not --mixed): the batch runs four legs in one process, without / with / without / with a
hot-phrase table of N random phrases of --phrase-len text tokens at boost 2 (State.set_phrase_table), one JSON line each and a
last line with the medians of the two settings and their difference per decoder step: what the boost kernel costs.
--repetition THETA,N (with --batch B, not --mixed, not with --hot-phrases): the same four legs without / with the repetition
rule (State.set_repeat_rule(THETA, N)): what the repetition kernel costs per decoder step.
--commands N (with --batch B, not --mixed, one at a time with the other two): the same four legs without / with a command list of
N random phrases of --phrase-len text tokens at penalty 100 (State.set_command_table): what the command-list kernel costs.
--out FILE appends the JSON line to FILE as well (profiles/).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from openhush_amd import engine as E, streaming as S, synth   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="large-v3")
    ap.add_argument("--chunk", type=float, default=5.0)
    ap.add_argument("--chunks", type=int, default=12)
    ap.add_argument("--beam", type=int, default=5)
    ap.add_argument("--tokens", type=int, default=48, help="decoder steps per chunk (synthetic weights never emit end-of-text by themselves)")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16"])
    ap.add_argument("--audio-ctx", default="0", help="0 (full context), N encoder positions, or auto (engine.audio_ctx_for of the chunk)")
    ap.add_argument("--batch", type=int, default=0, help="B > 0: B windows as one greedy batch instead of the streaming session")
    ap.add_argument("--reps", type=int, default=5, help="timed repetitions of the --batch run (after 2 warm-up runs)")
    ap.add_argument("--mixed", default=None, help="LO:HI seconds: per-window chunk lengths from a seeded uniform range (needs --batch)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the --mixed draw")
    ap.add_argument("--legs", default="ragged,envelope,off", help="legs of a --mixed run, comma separated: packed, ragged, envelope, off")
    ap.add_argument("--with-long", type=int, default=0, help="the first K windows of a --mixed batch are 30 s long")
    ap.add_argument("--hot-phrases", type=int, default=0, help="N > 0: A/B legs without and with a table of N random phrases (needs --batch)")
    ap.add_argument("--phrase-len", type=int, default=4, help="tokens per phrase of the --hot-phrases table")
    ap.add_argument("--repetition", default=None, metavar="THETA,N", help="A/B legs without and with the repetition rule (needs --batch)")
    ap.add_argument("--commands", type=int, default=0, help="N > 0: A/B legs without and with a command list of N random phrases (needs --batch)")
    ap.add_argument("--out", default=None, help="append the JSON result line to this file")
    a = ap.parse_args()

    def emit(rec):
        line = json.dumps(rec)
        print(line)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    ctx = E.Context.synthetic(synth.PRESETS[a.model].as_list(), 1234, 0, E.OHW_DTYPE_BF16 if a.dtype == "bf16" else E.OHW_DTYPE_F16)
    p = ctx.default_params()
    if a.beam >= 2:
        p.n_max = a.tokens          # beams end at n_max (force_len is the greedy loop's knob)
    else:
        p.force_len = a.tokens
    n = int(a.chunk * 16000)
    if a.mixed:
        if a.batch < 1:
            ap.error("--mixed needs --batch B")
        lo, hi = (float(x) for x in a.mixed.split(":"))
        secs = np.random.default_rng(a.seed).uniform(lo, hi, a.batch)
        secs[:max(0, min(a.with_long, a.batch))] = 30.0
        ns = [int(min(max(x, 0.1), 30.0) * 16000) for x in secs]
        lens = [min(E.audio_ctx_for(x), ctx.hp.n_audio_ctx) for x in ns]
        env = max(lens)
        st = E.State(ctx, a.batch)
        p.force_len = a.tokens
        pcm = np.zeros((a.batch, E.CHUNK_SAMPLES), np.float32)
        for b in range(a.batch):
            pcm[b, :ns[b]] = synth.synth_audio(40 + b)[:ns[b]]
        for leg in a.legs.split(","):
            if leg not in ("packed", "ragged", "envelope", "off"):
                ap.error("--legs: packed, ragged, envelope, off")
            st.set_audio_ctx(0 if leg == "off" else env)
            st.set_window_ctx(lens if leg in ("ragged", "packed") else None)
            st.set_packed_encoder(leg == "packed")
            enc, dec, wall, steps = [], [], [], 0
            for r in range(a.reps + 2):
                t0 = time.perf_counter()
                st.mel(pcm, ns, E.OHW_MEL_ZERO_TAIL, want=False)
                st.encode(a.batch)
                st.greedy(a.batch, p)
                t = st.timings()
                if r >= 2:
                    wall.append(time.perf_counter() - t0); enc.append(t.encode_ms); dec.append(t.decode_ms); steps = t.decode_steps
            E_ = st.audio_ctx
            emit({"workload": f"{a.model} batch of {a.batch} windows of {lo:g} .. {hi:g} s (seed {a.seed}), greedy, {a.tokens} decoder steps, {a.dtype}",
                  "leg": leg, "envelope": E_, "with_long": a.with_long, "enc_rows": st.counter("enc_rows"),
                  "sum_ctx_over_B_E": round(sum(lens) / (a.batch * E_), 4) if leg in ("ragged", "packed") else 1.0,
                  "sum_ctx2_over_B_E2": round(sum(x * x for x in lens) / (a.batch * E_ * E_), 4) if leg in ("ragged", "packed") else 1.0, "reps": a.reps,
                  "encode_ms": {"median": round(float(np.median(enc)), 3), "min": round(min(enc), 3), "max": round(max(enc), 3)},
                  "decode_ms_per_step": {"median": round(float(np.median(dec)) / max(1, steps), 4), "min": round(min(dec) / max(1, steps), 4),
                                         "max": round(max(dec) / max(1, steps), 4)},
                  "batch_latency_ms": {"median": round(1e3 * float(np.median(wall)), 2), "min": round(1e3 * min(wall), 2), "max": round(1e3 * max(wall), 2)}})
        return
    if a.batch > 0:
        n_ctx = E._audio_ctx_arg(a.audio_ctx)
        n_ctx = min(E.audio_ctx_for(n), ctx.hp.n_audio_ctx) if n_ctx < 0 else n_ctx
        st = E.State(ctx, a.batch)
        st.set_audio_ctx(n_ctx)
        p.force_len = a.tokens
        pcm = np.zeros((a.batch, E.CHUNK_SAMPLES), np.float32)
        for b in range(a.batch):
            pcm[b, :n] = synth.synth_audio(40 + b)[:n]
        rng = np.random.default_rng(a.seed)
        table = [[int(t) for t in rng.integers(0, ctx.tok.eot, a.phrase_len)] for _ in range(a.hot_phrases)]
        rule = None
        if a.repetition:
            if table:
                ap.error("--repetition and --hot-phrases are measured one at a time")
            theta, ngram = a.repetition.split(",")
            rule = (float(theta), int(ngram))
        if a.commands and (a.hot_phrases or rule):
            ap.error("--commands, --repetition and --hot-phrases are measured one at a time")
        commands = [[int(t) for t in rng.integers(0, ctx.tok.eot, a.phrase_len)] for _ in range(a.commands)]
        per_step = {0: [], 1: []}
        for leg in ([0, 1, 0, 1] if table or rule or commands else [0]):
            if commands:
                st.set_command_table(commands if leg else None, 100.0)
            elif rule:
                st.set_repeat_rule(*(rule if leg else (1.0, 0)))
            else:
                st.set_phrase_table(table if leg else None, 2.0)
            enc, dec, wall, steps = [], [], [], 0
            for r in range(a.reps + 2):
                t0 = time.perf_counter()
                st.mel(pcm, [n] * a.batch, E.OHW_MEL_ZERO_TAIL, want=False)
                st.encode(a.batch)
                st.greedy(a.batch, p)
                t = st.timings()
                if r >= 2:
                    wall.append(time.perf_counter() - t0); enc.append(t.encode_ms); dec.append(t.decode_ms); steps = t.decode_steps
            per_step[leg] += [d / max(1, steps) for d in dec]
            emit({"workload": f"{a.model} batch of {a.batch} windows of {a.chunk:g} s, greedy, {a.tokens} decoder steps, {a.dtype}",
                  "audio_ctx": st.audio_ctx, "gemm_small": os.environ.get("OHW_GEMM_SMALL", "default"), "reps": a.reps,
                  "hot_phrases": st.phrase_count(), "phrase_boost_launches": st.counter("phrase_boost"),
                  "repeat_rule": list(st.repeat_rule()), "repeat_rule_launches": st.counter("repeat_rule"),
                  "commands": st.command_count(), "command_rule_launches": st.counter("command_rule"),
                  "encode_ms": {"median": round(float(np.median(enc)), 3), "min": round(min(enc), 3), "max": round(max(enc), 3)},
                  "decode_ms_per_step": {"median": round(float(np.median(dec)) / max(1, steps), 4), "min": round(min(dec) / max(1, steps), 4),
                                         "max": round(max(dec) / max(1, steps), 4)},
                  "batch_latency_ms": {"median": round(1e3 * float(np.median(wall)), 2), "min": round(1e3 * min(wall), 2), "max": round(1e3 * max(wall), 2)}})
        if table or rule or commands:
            off, on = float(np.median(per_step[0])), float(np.median(per_step[1]))
            what = (f"command list of {a.commands} x {a.phrase_len} tokens, penalty 100" if commands else
                    f"repetition rule ({rule[0]:g}, {rule[1]})" if rule else f"hot-phrase table of {a.hot_phrases} x {a.phrase_len} tokens")
            emit({"workload": f"{a.model} batch of {a.batch}, greedy, {a.tokens} decoder steps, {a.dtype}: {what}",
                  "decode_ms_per_step_without": round(off, 4), "decode_ms_per_step_with": round(on, 4), "difference_us_per_step": round(1e3 * (on - off), 2),
                  "spread_us_without": round(1e3 * (max(per_step[0]) - min(per_step[0])), 2),
                  "spread_us_with": round(1e3 * (max(per_step[1]) - min(per_step[1])), 2), "runs_per_setting": len(per_step[0])})
        return
    rec = np.concatenate([synth.synth_audio(40 + i)[:n] for i in range(a.chunks)])
    vad = E.EnergyVad(-40.0)
    ses = S.StreamingSession(ctx, beam_size=a.beam, vad=vad, params=p, audio_ctx=a.audio_ctx)
    lat, enc, dec = [], [], []
    for i in range(a.chunks):
        job = ses.scheduler.tick(rec, (i + 1) * n)
        t0 = time.perf_counter()
        r = ses.transcribe_job(job)
        lat.append(time.perf_counter() - t0)
        t = ses.state.timings()
        enc.append(t.encode_ms); dec.append(t.decode_ms / max(1, t.decode_steps))
        ses.tracker.add_result(r)
        ses.tracker.take_ready()
    warm = lat[2:] or lat[-1:]        # the first chunks capture the two beam-step graphs (a one-chunk run - profiling - reports that chunk)
    emit({"workload": f"{a.model} streaming, {a.chunk:g} s chunks, beam {a.beam}, {a.tokens} decoder steps per chunk, {a.dtype}",
                      "audio_ctx": ses.state.audio_ctx, "gemm_small": os.environ.get("OHW_GEMM_SMALL", "default"),
                      "encode_ms": round(float(np.median(enc[2:] or enc[-1:])), 3), "decode_ms_per_step": round(float(np.median(dec[2:] or dec[-1:])), 4),
                      "first_chunk_ms": round(1e3 * lat[0], 2), "chunk_latency_ms": {"mean": round(1e3 * float(np.mean(warm)), 2),
                      "min": round(1e3 * min(warm), 2), "max": round(1e3 * max(warm), 2)},
                      "stream_real_time_factor": round(a.chunk / float(np.mean(warm)), 1), "silent_chunks_skipped": ses.skipped_silent})


if __name__ == "__main__":
    main()
