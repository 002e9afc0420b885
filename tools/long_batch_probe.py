"""What the long-form batch buys: N independent recordings of mixed lengths through whisper.cpp's seek loop, large-v3 dims,
synthetic model, bf16, the timestamp / end-of-text logit bias of the ladder tests (ts 6, eot 27) so that timestamps drive the
seeks.  Two legs on ONE engine, same recordings:

  A  ohw_engine_transcribe in OHW_WINDOW_SEEK once per recording (batch 1: the path a caller had before); a third leg repeats it
     with ohw_state_set_batch_invariant on, the mode leg B runs in
  B  ohw_engine_transcribe_long_batch (one window of every live recording per decode batch, up to --max-batch)

and, on a second engine of max_batch 1, leg B1 (B at one slot) against its own leg A1: the same windows one at a time through
the slot front end and the scheduler - a gap larger than A1's own min-max spread is what those two cost.

One warm-up and --repeats timed repeats per leg; median and min-max audio-s/s, the ratio of the medians, the round count and
the mean live batch size (replayed on ohw_seek_sched from the windows' seek deltas).  temperature_inc = 0 unless --ladder
(the default policy's fallback ladder, sampled on the device).  --carry turns the carried context on for every leg
(ohw_engine_set_carry_context(-1): every window after a recording's first pays a prefill); --chunk 16 runs those prefills in
16-position chunks.

  python tools/long_batch_probe.py [--recordings 32] [--min-s 45] [--max-s 300] [--max-batch 32] [--repeats 5] [--carry] [--chunk 8|16]
                                     [--json out.json]
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
    ap.add_argument("--recordings", type=int, default=32)
    ap.add_argument("--min-s", type=float, default=45.0)
    ap.add_argument("--max-s", type=float, default=300.0)
    ap.add_argument("--max-batch", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ladder", action="store_true", help="whisper.cpp's default policy with the device ladder instead of temperature_inc = 0")
    ap.add_argument("--carry", action="store_true", help="carried context on (set_carry_context(-1)) in every leg")
    ap.add_argument("--chunk", type=int, default=8, choices=[8, 16], help="positions per prefill chunk (set_prefill_chunk)")
    ap.add_argument("--skip-single-slot", action="store_true", help="leave out the max_batch = 1 engine (legs A1 / B1)")
    ap.add_argument("--budget-s", type=float, default=0.0,
                    help="give up before the timed legs when one pass of leg A, estimated from the first recording, would take longer "
                         "than this many seconds (0: no limit)")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats: at least five")

    from openhush_amd import engine as E, synth
    hp = synth.PRESETS["large-v3"]
    L = E.lib()
    # mixed lengths, evenly spread between the bounds and shuffled with a fixed seed; every recording its own audio
    rng = np.random.RandomState(7)
    secs = np.linspace(args.min_s, args.max_s, args.recordings)
    rng.shuffle(secs)
    pcms = []
    for i, s in enumerate(secs):
        n = int(round(s * 16000))
        wins = [synth.synth_audio(2000 + 16 * i + w) for w in range((n + synth.CHUNK_SAMPLES - 1) // synth.CHUNK_SAMPLES)]
        pcms.append(np.concatenate(wins)[:n].astype(np.float32))
    total_s = float(sum(len(p) for p in pcms)) / 16000.0

    def run_engine(max_batch, tag):
        pool = E.EnginePool(None, "en", False, [0], E.OHW_DTYPE_BF16, max_batch, synthetic=hp.as_list(), seed=1234)
        eng = E.WhisperEngine(C.c_void_p(L.ohw_pool_engine(pool.h, 0)))       # the pool owns it: never closed through the wrapper
        bias = np.zeros(hp.n_vocab, np.float32)
        tok = E.SpecialTokens()
        E._check(L.ohw_ctx_info(eng.ctx_h, C.byref(E.HParams()), C.byref(tok)))
        bias[tok.timestamp_begin:] = 6.0
        bias[tok.eot] = 27.0
        E._check(L.ohw_state_set_logit_bias(eng.state_h, E._fp(bias), bias.size))
        eng.set_decode_policy(temperature_inc=None if args.ladder else 0.0)
        eng.set_fallback_on_device(True)
        if args.carry:
            eng.set_carry_context(-1)
        eng.set_prefill_chunk(args.chunk)
        bufs = [E.AudioBuffer(p, 16000) for p in pcms]

        def leg_a():
            eng.set_window_mode(E.OHW_WINDOW_SEEK)
            t0 = time.perf_counter()
            toks = []
            for b in bufs:
                eng.transcribe(b)
                toks.append(eng.last_tokens())
            return time.perf_counter() - t0, toks

        def leg_a_invariant():
            # leg A with ohw_state_set_batch_invariant on, as inside leg B: what the kernel variants of that mode cost at batch 1
            E._check(L.ohw_state_set_batch_invariant(eng.state_h, 1))
            try:
                return leg_a()
            finally:
                E._check(L.ohw_state_set_batch_invariant(eng.state_h, 0))

        def leg_b():
            t0 = time.perf_counter()
            eng.transcribe_long_batch(bufs)
            dt = time.perf_counter() - t0
            return dt, [eng.batch_result(i)[1] for i in range(len(bufs))]

        def timed(fn):
            fn()                                                           # warm-up: allocations, graph captures
            ts, toks = [], None
            for _ in range(args.repeats):
                dt, toks = fn()
                ts.append(dt)
            rate = sorted(total_s / t for t in ts)
            return {"median_audio_s_per_s": statistics.median(rate), "min_audio_s_per_s": rate[0], "max_audio_s_per_s": rate[-1],
                    "wall_s": ts}, toks

        if args.budget_s > 0:
            eng.set_window_mode(E.OHW_WINDOW_SEEK)
            eng.transcribe(bufs[0])                                        # untimed: allocations
            t0 = time.perf_counter()
            eng.transcribe(bufs[0])
            est = (time.perf_counter() - t0) * total_s / bufs[0].duration_secs()
            print(f"[{tag}] recording 0: {len(eng.last_quality_ex())} windows for {bufs[0].duration_secs():.0f} s; one pass of leg A is estimated at {est:.1f} s", flush=True)
            if est > args.budget_s:
                print(f"[{tag}] NOT RUN: over the budget of {args.budget_s:.0f} s", flush=True)
                eng.h = None
                pool.close()
                sys.exit(3)
        a, toks_a = timed(leg_a)
        b, toks_b = timed(leg_b)
        ai, _ = timed(leg_a_invariant)
        # the rounds of leg B, replayed on the scheduler from the windows' own seek deltas
        deltas = [[q["seek_delta"] for q in eng.long_batch_quality(i)] for i in range(len(bufs))]
        sched, used, sizes = E.SeekSched([len(p) for p in pcms], max_batch), [0] * len(pcms), []
        while True:
            rnd = sched.round()
            if not rnd:
                break
            sizes.append(len(rnd))
            for k, (r, _, _, _) in enumerate(rnd):
                sched.advance(k, deltas[r][used[r]])
                used[r] += 1
        sched.close()
        out = {"max_batch": max_batch, "A_transcribe_seek_per_recording": a, "B_transcribe_long_batch": b, "A_with_batch_invariance_on": ai,
               "B_over_A_invariant": b["median_audio_s_per_s"] / ai["median_audio_s_per_s"],
               "B_over_A": b["median_audio_s_per_s"] / a["median_audio_s_per_s"],
               "A_spread": (a["max_audio_s_per_s"] - a["min_audio_s_per_s"]) / a["median_audio_s_per_s"],
               "rounds": len(sizes), "mean_live_batch": float(np.mean(sizes)) if sizes else 0.0, "windows": int(sum(sizes)),
               # batch invariance is on inside B and off inside A (one window per decode): the tokens may differ in last bits
               "recordings_with_equal_tokens": sum(1 for x, y in zip(toks_a, toks_b) if x == y)}
        print(f"[{tag}] max_batch {max_batch}: A {a['median_audio_s_per_s']:.1f} ({a['min_audio_s_per_s']:.1f} - {a['max_audio_s_per_s']:.1f}) audio-s/s, "
              f"B {b['median_audio_s_per_s']:.1f} ({b['min_audio_s_per_s']:.1f} - {b['max_audio_s_per_s']:.1f}) audio-s/s, B / A {out['B_over_A']:.2f}, "
              f"{out['rounds']} rounds, mean live batch {out['mean_live_batch']:.1f}, {out['windows']} windows; A with batch invariance on "
              f"{ai['median_audio_s_per_s']:.1f} ({ai['min_audio_s_per_s']:.1f} - {ai['max_audio_s_per_s']:.1f}), B / that {out['B_over_A_invariant']:.2f}", flush=True)
        eng.h = None
        pool.close()
        return out

    out = {"dims": "large-v3", "dtype": "bf16", "recordings": args.recordings, "seconds": [float(s) for s in secs], "audio_s": total_s,
           "repeats": args.repeats, "policy": "default, device ladder" if args.ladder else "temperature_inc 0", "bias": "ts 6 / eot 27",
           "carry": bool(args.carry), "prefill_chunk": args.chunk}
    out["batch"] = run_engine(args.max_batch, "batch")
    if not args.skip_single_slot:
        out["single_slot"] = run_engine(1, "single slot")
        g = out["single_slot"]
        g["gap"] = 1.0 - g["B_over_A"]
        print(f"[single slot] B1 against A1: gap {100 * g['gap']:.1f} %, A1's own spread {100 * g['A_spread']:.1f} %", flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
