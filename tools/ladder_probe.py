"""What the temperature fallback costs through the product path: ohw_engine_transcribe at large-v3 dims, bf16, host PCM in,
the default schedule and the DEFAULT decode policy (whisper.cpp's ladder T = 0.2 .. 1.0), three legs in one process:

  off     temperature_inc = 0: every window at T = 0 (what bench.py times)
  host    the host ladder (default): logits of the pending rows cross PCIe every step, ohw_sample_host samples them
  device  the device ladder (ohw_engine_set_fallback_device): ohw_sample_pass per rung, only tokens come back

on two workloads: the unbiased synthetic audio (every window fails through the repetition guard and runs all six passes)
and a timestamp / end-of-text logit bias (tests/test_gpu_policy.py _bias(6, 27); on micro most windows pass at T = 0) -
the share that fell back is measured, not assumed.  Per leg: audio-s/s, mean passes per window, the share of wall time spent
at T > 0 (against the off leg on the same windows).  The host leg runs fewer windows (--host-windows, default 32): it is slow.

  python tools/ladder_probe.py [--windows 120] [--host-windows 32] [--json out.json]

--best-of N measures best-of sampling instead (ohw_engine_set_best_of, ohw_sample_pass_n), same dims and dtype, unbiased audio
(every window runs every rung):

  rung        one rung at T = 0.6 for W = max_batch // N windows on one state, in the same process and alternating, every shape
              warmed first: ohw_sample_pass_n with N candidates per window, against N ohw_sample_pass rungs (what N candidates cost
              without the group pass) and against one ohw_sample_pass rung; median, minimum and maximum of --reps repetitions
  transcribe  ohw_engine_transcribe of --windows windows (default 24 in this mode) under the default policy with the device
              ladder, best_of 1 against best_of N: audio-s/s, the smaller T = 0 batch of best_of N included

  python tools/ladder_probe.py --best-of 5 [--max-batch 30] [--windows 24] [--reps 5] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def best_of_probe(args):
    from openhush_amd import engine as E, synth
    N = args.best_of
    hp = synth.PRESETS["large-v3"]
    W = max(1, args.max_batch // N)
    n_win = args.windows if args.windows != 120 else 24
    out = {"dims": "large-v3", "dtype": "bf16", "best_of": N, "max_batch": args.max_batch, "rung_windows": W, "temperature": 0.6, "reps": args.reps}
    ctx = E.Context.synthetic(hp.as_list(), 1234, 0, E.OHW_DTYPE_BF16)
    st = E.State(ctx, W * N)
    st.mel(np.stack([synth.synth_audio(1000 + w) for w in range(W)]), None, E.OHW_MEL_ZERO_TAIL, want=False)
    st.encode(W)
    p = ctx.default_params()
    cap = hp.n_text_ctx
    u = np.stack([np.stack([E.HostRng(j).uniforms(cap) for j in range(N)]) for _ in range(W)])
    act = [1] * W

    def group():
        return st.sample_pass_n(W, N, 0.6, act, u, p)

    def single(j):
        return st.sample_pass(W, 0.6, act, np.ascontiguousarray(u[:, j, :]), p)

    def timed(f):
        t0 = time.perf_counter()
        r = f()
        return time.perf_counter() - t0, r

    legs = {"group_n": group, "n_singles": lambda: [single(j) for j in range(N)], "one_single": lambda: single(0)}
    steps = {}
    for k, f in legs.items():                              # warm every shape: graph captures, first-use buffers
        _, r = timed(f)
        rows = r if k == "group_n" else (r[0] if k == "n_singles" else r)
        steps[k] = float(np.mean([len(x["tokens"]) + x["ended_by_eot"] for x in rows]))
    times = {k: [] for k in legs}
    for _ in range(args.reps):                             # alternating
        for k, f in legs.items():
            times[k].append(timed(f)[0])
    out["rung"] = {k: {"median_ms": 1e3 * float(np.median(v)), "min_ms": 1e3 * min(v), "max_ms": 1e3 * max(v), "mean_tokens_per_row": steps[k]} for k, v in times.items()}
    out["rung"]["group_vs_n_singles"] = out["rung"]["group_n"]["median_ms"] / out["rung"]["n_singles"]["median_ms"]
    out["rung"]["group_vs_one_single"] = out["rung"]["group_n"]["median_ms"] / out["rung"]["one_single"]["median_ms"]
    for k in legs:
        r = out["rung"][k]
        print(f"[rung, {W} windows, N = {N}] {k:>10}: median {r['median_ms']:8.1f} ms  (min {r['min_ms']:.1f}, max {r['max_ms']:.1f}; {r['mean_tokens_per_row']:.0f} tokens per row)", flush=True)
    print(f"[rung] group / N singles {out['rung']['group_vs_n_singles']:.3f}   group / one single {out['rung']['group_vs_one_single']:.3f}", flush=True)
    st.close()
    ctx.close()
    # through the product path
    pcm = np.concatenate([synth.synth_audio(1000 + w) for w in range(n_win)]).astype(np.float32)
    out["transcribe"] = {"windows": n_win}
    for bo in (1, N):
        pool = E.EnginePool(None, "en", False, [0], E.OHW_DTYPE_BF16, args.max_batch, synthetic=hp.as_list(), seed=1234)
        pool.set_fallback_on_device(True)
        pool.set_best_of(bo)
        audio = E.AudioBuffer(pcm, 16000)
        pool.transcribe(E.AudioBuffer(pcm[:min(n_win, max(1, args.max_batch // bo)) * synth.CHUNK_SAMPLES], 16000))      # warm-up: one batch
        ts = []
        for _ in range(2):
            t0 = time.perf_counter()
            pool.transcribe(audio)
            ts.append(time.perf_counter() - t0)
        out["transcribe"][f"best_of_{bo}"] = {"wall_s": ts, "audio_s_per_s": n_win * 30.0 / min(ts)}
        print(f"[transcribe, {n_win} windows, device ladder, all rungs] best_of {bo}: {n_win * 30.0 / min(ts):8.1f} audio-s/s  (walls {[round(t, 2) for t in ts]})", flush=True)
        pool.close()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=120, help="windows of the off / device legs (config #4: 120 = 1 h)")
    ap.add_argument("--host-windows", type=int, default=32, help="windows of the host leg (and of its off leg)")
    ap.add_argument("--max-batch", type=int, default=32)
    ap.add_argument("--json", default="")
    ap.add_argument("--best-of", type=int, default=0, help="measure best-of sampling with N candidates instead (see above)")
    ap.add_argument("--reps", type=int, default=5, help="--best-of: repetitions of every rung leg")
    args = ap.parse_args()
    if args.best_of:
        if not 2 <= args.best_of <= 5 or args.max_batch < args.best_of:
            ap.error("--best-of takes 2..5 and a --max-batch of at least that")
        return best_of_probe(args)

    from openhush_amd import engine as E, synth
    hp = synth.PRESETS["large-v3"]
    pool = E.EnginePool(None, "en", False, [0], E.OHW_DTYPE_BF16, args.max_batch, synthetic=hp.as_list(), seed=1234)
    L = E.lib()
    eng = C.c_void_p(L.ohw_pool_engine(pool.h, 0))
    state = C.c_void_p(L.ohw_engine_state(eng))
    hpc, tok = E.HParams(), E.SpecialTokens()
    E._check(L.ohw_ctx_info(C.c_void_p(L.ohw_engine_ctx(eng)), C.byref(hpc), C.byref(tok)))
    n_win = max(args.windows, args.host_windows)
    pcm = np.concatenate([synth.synth_audio(1000 + w) for w in range(n_win)]).astype(np.float32)
    bias = np.zeros(hp.n_vocab, np.float32)
    bias[tok.timestamp_begin:] = 6.0
    bias[tok.eot] = 27.0

    def policy(inc):
        pol = E.DecodePolicy()
        L.ohw_default_decode_policy(C.byref(pol))
        if inc is not None:
            pol.temperature_inc = inc
        E._check(L.ohw_engine_set_decode_policy(eng, C.byref(pol)))

    def transcribe(nw):
        x = pcm[:nw * synth.CHUNK_SAMPLES]
        buf = C.create_string_buffer(64)
        t0 = time.perf_counter()
        E._check(L.ohw_engine_transcribe(eng, E._fp(x), x.size, 16000, buf, len(buf), None, None, None))
        dt = time.perf_counter() - t0
        q, n = C.POINTER(E.WindowQuality)(), C.c_int(0)
        E._check(L.ohw_engine_last_quality(eng, C.byref(q), C.byref(n)))
        fell_back = sum(1 for i in range(n.value) if q[i].would_fallback)
        kept_t = [round(float(q[i].temperature), 1) for i in range(n.value)]
        tr, m = C.POINTER(C.c_int32)(), C.c_int(0)
        E._check(L.ohw_engine_last_trace(eng, C.byref(tr), C.byref(m)))
        data = np.ctypeslib.as_array(tr, shape=(m.value,)) if m.value else np.zeros(0, np.int32)
        passes, i = 0, 0
        while i + 3 <= len(data):
            passes += 1
            i += 3 + int(data[i + 2])
        return {"windows": nw, "wall_s": dt, "audio_s_per_s": nw * 30.0 / dt, "passes_per_window": passes / nw,
                "fell_back_share": fell_back / nw, "kept_temperatures": {str(t): kept_t.count(t) for t in sorted(set(kept_t))}}

    def leg(name, nw, inc, on_device):
        policy(inc)
        E._check(L.ohw_engine_set_fallback_device(eng, 1 if on_device else 0))
        r = transcribe(nw)
        r["leg"] = name
        return r

    out = {"dims": "large-v3", "dtype": "bf16", "max_batch": args.max_batch, "schedule": "default", "policy": "default",
           "host_leg_windows": args.host_windows, "workloads": {}}
    leg("warm-up", args.windows, 0.0, False)                 # states, lanes, graph captures
    for wl, b in (("unbiased (all windows fail)", None), ("bias ts 6 / eot 27", bias)):
        E._check(L.ohw_state_set_logit_bias(state, E._fp(b) if b is not None else C.cast(None, C.POINTER(C.c_float)), hp.n_vocab if b is not None else 0))
        rs = {}
        rs["off"] = leg("off", args.windows, 0.0, False)
        rs["device"] = leg("device", args.windows, None, True)
        rs["off_host_windows"] = leg("off", args.host_windows, 0.0, False)
        rs["host"] = leg("host", args.host_windows, None, False)
        for k, base in (("device", "off"), ("host", "off_host_windows")):
            rs[k]["t_gt0_share"] = max(0.0, 1.0 - rs[base]["wall_s"] / rs[k]["wall_s"])
        rs["device_vs_host_audio_s_per_s"] = rs["device"]["audio_s_per_s"] / rs["host"]["audio_s_per_s"]
        rs["ladder_on_vs_off_device"] = rs["device"]["audio_s_per_s"] / rs["off"]["audio_s_per_s"]
        out["workloads"][wl] = rs
        for k in ("off", "device", "off_host_windows", "host"):
            r = rs[k]
            print(f"[{wl}] {k:>16}: {r['windows']:4d} windows  {r['audio_s_per_s']:9.1f} audio-s/s  {r['passes_per_window']:.2f} passes/window  "
                  f"fell back {100 * r['fell_back_share']:.0f} %" + (f"  T > 0 share of wall {100 * r['t_gt0_share']:.0f} %" if "t_gt0_share" in r else ""),
                  flush=True)
        print(f"[{wl}] device / host ladder: {rs['device_vs_host_audio_s_per_s']:.2f}x   device ladder on / off: {rs['ladder_on_vs_off_device']:.3f}"
              f"   (host leg on {args.host_windows} windows, others on {args.windows})", flush=True)
    E._check(L.ohw_engine_set_fallback_device(eng, 0))
    pool.close()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
