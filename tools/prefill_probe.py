"""Time ohw_state_prefill: a 224-position context at large-v3 dimensions, OHW_PREFILL_XA=1 against =0.

    python tools/prefill_probe.py [--windows 1,32,96] [--cus 64] [--preset large-v3] [--runs 5] [--chunk 8|16] [--out FILE.json]

For every window count and both knob values (each in a child process: the knob is read when a state is created) it reports the
median of --runs timed prefills after one warm-up, and from ohw_state_profile_begin / _end the time inside the cross-attention
launches and inside the decoder GEMM launches of one prefill.  The windows are bench.py's kind (synthetic recordings through mel
and encoder); a batch above 32 windows runs on a stream masked to --cus compute units, as a lane of the LANES schedule does.
OHW_PREFILL_XA=0 is the parent commit's kernels on the same chunks.  A prefill ends with a stream synchronisation, so it is
timed with the host's clock around the call (tens of milliseconds and more: the call's overhead does not show).
K/V bytes per chunk = 2 (K, V) * layers * windows * heads * keys * 64 * 2 bytes; the rate is those bytes times the chunks over the
cross-attention time, to be read against the 5.7 TB/s the single-token kernel reaches.
--chunk 8|16 times the prefill at that chunk size (ohw_state_set_prefill_chunk) with the knob at its default alone, one process per
window count: chunk 8 is the unchanged path and the baseline of chunk 16.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(preset, windows, cus, runs, chunk):
    import numpy as np
    from openhush_amd import engine as E, synth
    hp = synth.PRESETS[preset]
    ctx = E.Context.synthetic(hp.as_list(), 1234, 0, E.OHW_DTYPE_BF16)
    st = E.State(ctx, windows)
    st.set_prefill_chunk(chunk)
    stream = None
    if windows > 32 and cus > 0:
        stream = E.Stream(0, 0, cus)
        st.set_stream(stream.ptr)
    for b0 in range(0, windows, 8):          # the front end in slices of 8 windows keeps the host buffer small
        n = min(8, windows - b0)
        pcm = np.stack([synth.synth_audio(b0 + i) for i in range(n)])
        st.mel(pcm, None, E.OHW_MEL_ZERO_TAIL, want=False)
        st.encode_slice(n, b0, windows)
    cap = hp.n_text_ctx // 2 - 1
    rng = np.random.default_rng(3)
    st.set_window_prompt([[int(t) for t in rng.integers(0, ctx.tok.eot, size=cap)] for _ in range(windows)])
    st.prefill(windows)                      # warm-up
    times = []
    for _ in range(runs):
        t0 = time.perf_counter()
        st.prefill(windows)
        times.append(1e3 * (time.perf_counter() - t0))
    prof = {}
    for name, cls in (("xattn", 3), ("gemm", 4), ("gemm_qkv", 5), ("gemm_xq", 6), ("gemm_fc1", 7)):
        st.profile_begin(cls)
        st.prefill(windows)
        n, ms, _ = st.profile_end()
        prof[name] = {"launches": n, "ms": ms}
    chunks = (cap + 1 + chunk - 1) // chunk
    kv_chunk = 2.0 * hp.n_text_layer * windows * hp.n_text_head * hp.n_audio_ctx * 64 * 2
    xa_ms = prof["xattn"]["ms"]
    print(json.dumps({"windows": windows, "chunk": chunk, "xa": int(os.environ.get("OHW_PREFILL_XA", "1")), "cus": cus if stream else 0,
                      "prefill_ms_median": statistics.median(times), "prefill_ms": times, "chunks": chunks,
                      "xattn_launches_chunk_kernel": st.counter("xattn.chunk"), "profile": prof,
                      "gemm_ms_all": sum(prof[k]["ms"] for k in prof if k != "xattn"),
                      "kv_gb_per_chunk": kv_chunk / 1e9, "kv_tb_per_s": (kv_chunk * chunks / (xa_ms * 1e-3) / 1e12) if xa_ms > 0 else None}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", default="1,32,96")
    ap.add_argument("--cus", type=int, default=64)
    ap.add_argument("--preset", default="large-v3")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=0, choices=[0, 8, 16], help="0 (default): chunk 8 under both values of OHW_PREFILL_XA")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        child(a.preset, a.child, a.cus, a.runs, a.chunk or 8)
        return 0
    rows = []
    for w in [int(x) for x in a.windows.split(",")]:
        for xa in ("1", "0") if a.chunk == 0 else ("1",):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(w), "--cus", str(a.cus), "--preset", a.preset, "--runs", str(a.runs),
                                "--chunk", str(a.chunk or 8)],
                               env=dict(os.environ, OHW_PREFILL_XA=xa), capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                print(r.stdout[-2000:], r.stderr[-2000:], file=sys.stderr)
                return 1            # nothing more is started on the device after a failure
            row = json.loads(r.stdout.strip().splitlines()[-1])
            rows.append(row)
            print(f"windows {w:3d} chunk {row['chunk']} xa={xa}: prefill {row['prefill_ms_median']:.1f} ms (median of {a.runs}); cross-attention {row['profile']['xattn']['ms']:.1f} ms, "
                  f"GEMMs {row['gemm_ms_all']:.1f} ms; K/V {row['kv_gb_per_chunk']:.2f} GB per chunk, {row['kv_tb_per_s'] or 0:.2f} TB/s", flush=True)
            if a.out:
                with open(a.out, "w") as f:
                    json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
