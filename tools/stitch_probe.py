"""What stitched windows cost: one recording of --windows fixed cuts (default 60 = 30 minutes) under the LANES schedule, large-v3
dims, synthetic model, bf16, --tokens tokens per window (end-of-text suppressed, as bench.py decodes).  Legs on ONE engine:

  off      ohw_engine_transcribe with stitch off (on a parent checkout, whose library has no ohw_engine_set_stitch, the only leg:
           run the script there for the parent's figure and its run-to-run spread)
  stitch   the same recording with ohw_engine_set_stitch(--overlap seconds): 30 / (30 - overlap) times the windows

and, on the window tokens the stitched leg produced, the time of ohw_stitch_seams (device: allocation, two copies in, launch,
copy out) against ohw_stitch_seams_host, plus the two on a table of an hour at a 25 s hop (143 seams of 225 text tokens a side).

One warm-up and --repeats timed repeats per leg: median and min-max audio-s/s.

  python tools/stitch_probe.py [--windows 60] [--overlap 5] [--max-batch 32] [--tokens 100] [--repeats 5] [--json out.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=60)
    ap.add_argument("--overlap", type=float, default=5.0)
    ap.add_argument("--max-batch", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats: at least five")

    from openhush_amd import engine as E, synth
    hp = synth.PRESETS["large-v3"]
    L = E.lib()
    has_stitch = hasattr(L, "ohw_engine_set_stitch")
    pcm = np.concatenate([synth.synth_audio(3000 + w) for w in range(args.windows)]).astype(np.float32)
    audio_s = len(pcm) / 16000.0
    buf = E.AudioBuffer(pcm, 16000)
    pool = E.EnginePool(None, "en", False, [0], E.OHW_DTYPE_BF16, args.max_batch, synthetic=hp.as_list(), seed=1234)
    eng = E.WhisperEngine(C.c_void_p(L.ohw_pool_engine(pool.h, 0)))       # the pool owns it: never closed through the wrapper
    eng.set_decode_policy(temperature_inc=0.0, no_speech_thold=2.0)
    eng.set_force_len(args.tokens)
    eng.set_schedule(E.OHW_SCHEDULE_LANES)

    def timed(fn, repeats):
        fn()                                                               # warm-up: allocations, graph captures
        ts = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return ts

    def leg(tag):
        ts = timed(lambda: eng.transcribe(buf), args.repeats)
        rate = sorted(audio_s / t for t in ts)
        out = {"median_audio_s_per_s": statistics.median(rate), "min_audio_s_per_s": rate[0], "max_audio_s_per_s": rate[-1], "wall_s": ts,
               "windows": len(eng.last_quality_ex())}
        print(f"[{tag}] {out['windows']} windows: {out['median_audio_s_per_s']:.1f} ({rate[0]:.1f} - {rate[-1]:.1f}) audio-s/s", flush=True)
        return out

    def seam_times(tag, windows):
        tok, n_text, _ = E._stitch_table(windows)
        dev = timed(lambda: E.stitch_seams((tok, n_text)), 20)
        host = timed(lambda: E.stitch_seams_host((tok, n_text)), 20)
        assert (E.stitch_seams((tok, n_text)) == E.stitch_seams_host((tok, n_text))).all()
        out = {"seams": len(n_text) - 1, "mean_text_tokens": float(np.mean(n_text)), "device_ms_median": 1e3 * statistics.median(dev),
               "device_ms_min": 1e3 * min(dev), "host_ms_median": 1e3 * statistics.median(host), "host_ms_min": 1e3 * min(host)}
        print(f"[{tag}] {out['seams']} seams of {out['mean_text_tokens']:.0f} text tokens a side: ohw_stitch_seams {out['device_ms_median']:.3f} ms, "
              f"ohw_stitch_seams_host {out['host_ms_median']:.3f} ms (medians of 20)", flush=True)
        return out

    out = {"dims": "large-v3", "dtype": "bf16", "audio_s": audio_s, "max_batch": args.max_batch, "tokens_per_window": args.tokens,
           "repeats": args.repeats, "schedule": "lanes", "library_has_stitch": has_stitch}
    out["off"] = leg("off")
    if has_stitch:
        eng.set_stitch(args.overlap)
        out["stitch"] = leg(f"stitch {args.overlap:g} s")
        out["stitch"]["overlap_s"] = args.overlap
        out["stitch_over_off"] = out["stitch"]["median_audio_s_per_s"] / out["off"]["median_audio_s_per_s"]
        out["windows_ratio"] = out["stitch"]["windows"] / out["off"]["windows"]
        eot = E.SpecialTokens()
        E._check(L.ohw_ctx_info(eng.ctx_h, C.byref(E.HParams()), C.byref(eot)))
        wins = [[t for t in w if t < eot.eot] for w in eng.last_window_tokens()]
        out["seams_of_the_call"] = seam_times("the call's seams", wins)
        # an hour at a 25 s hop: 144 windows of 225 text tokens, neighbours sharing their last / first 37
        rng = np.random.default_rng(1)
        hour = [[int(x) for x in rng.integers(0, 50000, 225)] for _ in range(144)]
        for w in range(1, 144):
            hour[w][:37] = hour[w - 1][-37:]
        out["seams_of_an_hour"] = seam_times("an hour at a 25 s hop", hour)
        eng.set_stitch(0)
        out["off_again"] = leg("off again")
    eng.h = None
    pool.close()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
