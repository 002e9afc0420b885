"""What the speech-aware windows cost and buy.  Two measurements, three timed runs each after one warm-up, median and min-max:

  detector   ohw_state_vad_frames on --hours of synthetic audio (noise at -60 dBFS, tone bursts at -20 dBFS), samples on the host
             (the call stages them) and resident on the device (the three kernels and the read-back alone), against the same rule
             in numpy on the host (fp32 matrix products over blocks of frames; timed on --host-minutes and scaled to an hour)
  engine     one --minutes recording, half of it silence (bursts of --burst-s every 2 * --burst-s), large-v3 dims, synthetic
             model, bf16, the timestamp / end-of-text bias of tools/long_batch_probe.py:
               S  ohw_engine_transcribe_speech under the auto audio context with the packed encoder
               L  ohw_engine_transcribe_long_batch on the same recording (the seek loop, full context: the path before)
             audio-s/s of both and the decoder rows each ran (S: chunks; L: windows)

  python tools/vad_probe.py [--hours 1] [--host-minutes 10] [--minutes 10] [--burst-s 15] [--max-batch 32] [--skip-engine] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RUNS = 3


def burst_audio(seconds, burst_s, seed=7):
    """noise at -60 dBFS; four modulated tones at -20 dBFS during the first burst_s of every 2 * burst_s"""
    n = int(round(seconds * 16000))
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * 1e-3).astype(np.float32)
    period = int(round(2 * burst_s * 16000))
    t = np.arange(period, dtype=np.float64) / 16000.0
    tone = sum(np.sin(2 * np.pi * f * t + 0.3 * i) for i, f in enumerate((440.0, 880.0, 1320.0, 2200.0))) / 4
    tone *= 0.1 * np.sqrt(8.0) * (1.0 + 0.3 * np.sin(2 * np.pi * 4.0 * t)) / 1.3
    tone[period // 2:] = 0.0
    tone[:8000] = 0.0                                       # every recording starts with half a second of noise
    reps = (n + period - 1) // period
    x += np.tile(tone.astype(np.float32), reps)[:n]
    return x


def host_rule(x, q=0.10, margin=9.0, slope=3.0, block=20000):
    """the detector's three rules in numpy, fp32: -> probabilities per 10 ms frame"""
    n = len(x)
    nf = (n + 159) // 160
    j = np.arange(400)
    win = (0.5 - 0.5 * np.cos(2 * np.pi * j / 400)).astype(np.float32)
    ang = 2 * np.pi * np.outer(j, np.arange(8, 86)) / 400
    cs = np.concatenate([np.cos(ang), -np.sin(ang)], axis=1).astype(np.float32)        # [400][156]
    xz = np.concatenate([x, np.zeros(1, np.float32)])
    e = np.empty(nf, np.float32)
    for t0 in range(0, nf, block):
        t = np.arange(t0, min(t0 + block, nf))[:, None]
        pos = np.abs(t * 160 - 200 + j[None, :])
        fr = xz[np.minimum(pos, n)] * win[None, :]
        X = fr @ cs
        e[t0:t0 + len(t)] = 10.0 * np.log10(np.maximum((X * X).sum(axis=1), 1e-10))
    bins = np.clip(np.floor((e + np.float32(100)) * np.float32(2)), 0, 319).astype(np.int64)
    cum = np.cumsum(np.bincount(bins, minlength=320))
    target = min(max(int(np.ceil(np.float32(q) * np.float32(nf))), 1), nf)
    floor = -100.0 + 0.5 * int(np.argmax(cum >= target))
    c = np.concatenate([np.zeros(1), np.cumsum(e.astype(np.float64))])
    a, b = np.maximum(np.arange(nf) - 2, 0), np.minimum(np.arange(nf) + 2, nf - 1)
    es = (c[b + 1] - c[a]) / (b - a + 1)
    return (1.0 / (1.0 + np.exp(-(es - floor - margin) / slope))).astype(np.float32), floor


def three(fn):
    fn()
    ts = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hours", type=float, default=1.0)
    ap.add_argument("--host-minutes", type=float, default=10.0)
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--burst-s", type=float, default=15.0)
    ap.add_argument("--max-batch", type=int, default=32)
    ap.add_argument("--skip-engine", action="store_true")
    ap.add_argument("--json", default="")
    args = ap.parse_args()

    import torch
    from openhush_amd import engine as E, synth
    L = E.lib()
    out = {"runs": RUNS}

    # ---- detector ----
    ctx = E.Context.synthetic(synth.PRESETS["nano"].as_list(), 1234, 0, E.OHW_DTYPE_BF16)
    st = E.State(ctx, 1)
    x = burst_audio(args.hours * 3600.0, args.burst_s)
    per_hour = 3600.0 / (len(x) / 16000.0)
    dev = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    p_host_pcm, fl = st.vad_frames(x)
    p_dev_pcm, _ = st.vad_frames(dev.data_ptr(), len(x))
    assert p_host_pcm.tobytes() == p_dev_pcm.tobytes()
    d_host = three(lambda: st.vad_frames(x))
    d_dev = three(lambda: st.vad_frames(dev.data_ptr(), len(x)))
    del dev
    xh = x[:int(args.host_minutes * 60 * 16000)]
    p_np, fl_np = host_rule(xh)
    p_gpu, fl_gpu = st.vad_frames(xh)
    h = three(lambda: host_rule(xh))
    scale = 3600.0 / (len(xh) / 16000.0)
    out["detector"] = {"audio_s": len(x) / 16000.0, "floor_db": fl,
                       "device_host_pcm_s_per_hour": {k: v * per_hour for k, v in d_host.items()},
                       "device_resident_pcm_s_per_hour": {k: v * per_hour for k, v in d_dev.items()},
                       "numpy_s_per_hour": {k: v * scale for k, v in h.items()}, "numpy_timed_on_s": len(xh) / 16000.0,
                       "numpy_vs_device_max_abs_p": float(np.abs(p_np - p_gpu).max()), "numpy_floor_db": fl_np, "device_floor_db": fl_gpu}
    print("[detector]", json.dumps(out["detector"]), flush=True)
    st.close()
    ctx.close()

    # ---- engine ----
    if not args.skip_engine:
        hp = synth.PRESETS["large-v3"]
        pool = E.EnginePool(None, "en", False, [0], E.OHW_DTYPE_BF16, args.max_batch, synthetic=hp.as_list(), seed=1234)
        eng = E.WhisperEngine(C.c_void_p(L.ohw_pool_engine(pool.h, 0)))       # the pool owns it: never closed through the wrapper
        bias = np.zeros(hp.n_vocab, np.float32)
        tok = E.SpecialTokens()
        E._check(L.ohw_ctx_info(eng.ctx_h, C.byref(E.HParams()), C.byref(tok)))
        bias[tok.timestamp_begin:] = 6.0
        bias[tok.eot] = 27.0
        E._check(L.ohw_state_set_logit_bias(eng.state_h, E._fp(bias), bias.size))
        eng.set_decode_policy(temperature_inc=0.0)
        rec = E.AudioBuffer(burst_audio(args.minutes * 60.0, args.burst_s, seed=9), 16000)
        audio_s = rec.duration_secs()

        def leg_s():
            eng.set_audio_ctx("auto")
            eng.set_packed_encoder(True)
            eng.transcribe_speech([rec])

        def leg_l():
            eng.set_audio_ctx(0)
            eng.set_packed_encoder(False)
            eng.transcribe_long_batch([rec])
        s = three(leg_s)
        chunks = eng.speech_chunks(0)
        s_tokens = len(eng.batch_result(0)[1])
        l = three(leg_l)
        windows = len(eng.long_batch_quality(0))
        l_tokens = len(eng.batch_result(0)[1])
        rate = lambda d: {"median_audio_s_per_s": audio_s / d["median_s"], "min_audio_s_per_s": audio_s / d["max_s"], "max_audio_s_per_s": audio_s / d["min_s"]}
        out["engine"] = {"dims": "large-v3", "dtype": "bf16", "audio_s": audio_s, "max_batch": args.max_batch, "bias": "ts 6 / eot 27",
                         "S_transcribe_speech_auto_packed": dict(rate(s), decoder_rows=len(chunks), tokens=s_tokens,
                                                                 chunk_seconds=[(c["end"] - c["start"]) / 16000.0 for c in chunks]),
                         "L_transcribe_long_batch": dict(rate(l), decoder_rows=windows, tokens=l_tokens)}
        out["engine"]["S_over_L"] = out["engine"]["S_transcribe_speech_auto_packed"]["median_audio_s_per_s"] / out["engine"]["L_transcribe_long_batch"]["median_audio_s_per_s"]
        print("[engine]", json.dumps(out["engine"]), flush=True)
        eng.h = None
        pool.close()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
