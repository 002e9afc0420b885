"""The decoder step against the fp32 oracle over the whole text context (positions 0 .. 447) and in every kernel variant the
default path picks.

The oracle is fed the GPU's OWN encoder output (st.fetch("enc") -> oracle.State.set_encoder_output): a logit error measured
here is the decoder's alone, and the large-v3 cases skip the oracle's encoder.

Tolerances (those of tests/test_gpu_parity.py, not loosened here):
  logits, micro dims      sigma ~ 4             : bf16 0.25 / f16 0.03 abs
  logits, large-v3 dims   bf16 and f16          : 0.07 sigma (the large-v3 bound of test_gpu_parity.py)
  picks                   argmax equal, or the oracle's own top-2 margin within twice the logit tolerance
  opt-in variants         OHW_DEC_FUSE_ATTN=1: the separate launch's bits; the persistent step: the f16 logit tolerance
                          against the launch path (tests/test_gpu_fused_attn.py, tests/test_gpu_persist.py)

Which variant a call launched is read from the state's host-side tally (ohw_dbg_counter "dec_gemm.*", "xattn.*",
"self_attn.*", include/ohw.h).
"""
import os
import time

import numpy as np
import pytest

from openhush_amd import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOL_LOGIT = {0: 0.25, 1: 0.03}
N_CTX = 448
BUCKET = 64


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from openhush_amd import engine
    engine.lib()
    return engine


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o
    o.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    return o


def _tokens(tok, seed, n=N_CTX):
    """tools/gen_golden.py's pattern: [sot, lang, transcribe, timestamp_begin], then random text ids with increasing
    timestamp tokens mixed in - every position sees another token"""
    rng = np.random.default_rng(seed)
    seq = [tok.sot, tok.sot + 1, tok.transcribe, tok.timestamp_begin]
    ts = 0
    while len(seq) < n:
        if rng.random() < 0.1:
            ts = min(ts + int(rng.integers(1, 12)), 1500)
            seq.append(tok.timestamp_begin + ts)
        else:
            seq.append(int(rng.integers(0, tok.eot)))
    return seq


def _tally(st):
    """every decoder-variant counter of the state that is non-zero"""
    names = [f"dec_gemm.{g}{f}.{s}" for g in ("qkv", "o", "xq", "xo", "fc1", "fc2", "logits") for f in ("", ".ln", ".pn", ".ks")
             for s in ("1x1", "2x1", "1x2", "2x2", "4x2")]
    names += ["xattn." + v for v in ("plain", "split", "rows2", "rows3", "rows4", "group2", "group3", "group4", "group5", "group_split")]
    names += ["self_attn." + v for v in ("plain", "slots", "fused", "fused_slots")]
    out = {}
    for n in names:
        v = st.counter(n)
        if v:
            out[n] = v
    return out


def _delta(after, before):
    return {k: v - before.get(k, 0) for k, v in after.items() if v - before.get(k, 0) > 0}


def _check_row(got, ref, tol, where):
    err = float(np.abs(got - ref).max())
    assert err < tol, (where, err)
    if int(got.argmax()) != int(ref.argmax()):
        top = np.sort(ref)[-2:]
        assert top[1] - top[0] < 2 * tol, (where, int(got.argmax()), int(ref.argmax()), float(top[1] - top[0]))
    return err


def _buckets(worst):
    return " ".join(f"{i * BUCKET}-{min(N_CTX, (i + 1) * BUCKET) - 1}: {w:.4f}" for i, w in enumerate(worst))


# ---------------------------------------------------------------------------------------------------------------------
# (a) the depth sweep: three windows, teacher-forced from position 0 to 447, rows at different positions in one call
# ---------------------------------------------------------------------------------------------------------------------
# Row r follows a clock with lag LAGS[r] (row 2 leads row 0 by 64, row 1 trails row 0 by one): one call feeds row 0 at 64,
# row 1 at 63 and row 2 at 128.  A row whose clock has not moved re-feeds tokens it already fed (same K/V rewritten).
# BURSTS: (row, position) -> n_new: that row advances n_new tokens in one call while the others wait; a waiting row then
# re-feeds an already-fed window across 63|64 or 127|128, so every multi-token call crosses both chunk edges.  The row that
# reaches 440 last feeds 440..447 in one call (ohw_decode's position rule: n_past + n_new <= 448).
LAGS = (64, 65, 0)
BURSTS = {(2, 63): 2, (1, 61): 4, (2, 121): 8, (0, 126): 3, (2, 250): 2, (2, 300): 3, (2, 350): 4, (2, 400): 8}


def _schedule():
    """[(n_new, [n_past per row])] - pure host arithmetic"""
    p = [4, 4, 4]
    calls = [(4, [0, 0, 0])]
    c = 4
    while min(p) < N_CTX:
        due = [p[r] + 1 <= min(N_CTX, c + 1 - LAGS[r]) for r in range(3)]
        last = min(range(3), key=lambda r: p[r])
        burst = [r for r in range(3) if (r, p[r]) in BURSTS and due[r]]
        if p[last] == N_CTX - 8 and due[last]:
            k, lead = 8, last
        elif burst:
            k, lead = BURSTS[(burst[0], p[burst[0]])], burst[0]
        else:
            k, lead = 1, None
            c += 1
        adv = [p[r] + 1 <= min(N_CTX, c - LAGS[r]) for r in range(3)] if lead is None else [r == lead for r in range(3)]
        npst, edges = [], [64, 128]
        for r in range(3):
            if adv[r]:
                npst.append(p[r])
                continue
            q = max(0, p[r] - k)
            for e in list(edges) if k > 1 else []:
                if e - (k + 1) // 2 + k <= p[r]:
                    q = e - (k + 1) // 2
                    edges.remove(e)
                    break
            npst.append(q)
        for r in range(3):
            p[r] += k if adv[r] else 0
        calls.append((k, npst))
    return calls


def _schedule_properties(calls):
    cross, together = {}, False
    for k, npst in calls:
        for n in npst:
            for e in (63, 127):
                if n <= e < n + k - 1:
                    cross.setdefault(k, set()).add(e)
        last = sorted(n + k - 1 for n in npst)
        together = together or (63 in last and 64 in last and last[-1] >= 127)
    return cross, together


def _sweep(E, st, seqs, on_call):
    """feed the schedule; on_call(call index, n_past list, n_new, logits) for every call"""
    for i, (k, npst) in enumerate(_schedule()):
        toks = np.asarray([seqs[r][npst[r]:npst[r] + k] for r in range(3)], np.int32)
        on_call(i, npst, k, st.decode(toks, npst))


def _depth_setup(E, oracle, tmp_models, preset, dt, seed0=40):
    path = tmp_models(preset)
    om = oracle.Model.load(path)
    ctx = E.Context.from_file(path, 0, dt)
    st = E.State(ctx, 3)
    st.mel(np.stack([synth.synth_audio(seed0 + r) for r in range(3)]), None, E.OHW_MEL_ZERO_TAIL, want=False)
    st.encode(3)
    seqs = [_tokens(ctx.tok, 1000 + r) for r in range(3)]
    return om, ctx, st, seqs


def test_depth_schedule_covers_the_chunk_edges():
    """the sweep's schedule (host arithmetic) does what the depth tests rely on"""
    calls = _schedule()
    cross, together = _schedule_properties(calls)
    for k in (2, 3, 4, 8):
        assert cross.get(k, set()) >= {63, 127}, (k, cross)
    assert together
    fed = [set() for _ in range(3)]
    for k, npst in calls:
        for r in range(3):
            assert 0 <= npst[r] and npst[r] + k <= N_CTX
            fed[r].update(range(npst[r], npst[r] + k))
    assert all(f == set(range(N_CTX)) for f in fed)
    assert any(k == 8 and N_CTX - 8 in npst for k, npst in calls)         # a row's last call: positions 440 .. 447


@pytest.mark.parametrize("preset", ["micro", "micro-v3"])
@pytest.mark.parametrize("dt", [0, 1])
def test_teacher_forced_logits_at_every_depth(E, oracle, tmp_models, preset, dt):
    om, ctx, st, seqs = _depth_setup(E, oracle, tmp_models, preset, dt)
    enc = st.fetch("enc", 3)
    ref = []
    for r in range(3):
        s = oracle.State(om)
        s.set_encoder_output(enc[r])
        ref.append(s.decode(seqs[r], 0, all_pos=True))
        s.close()
    tol = TOL_LOGIT[dt]
    worst = [0.0] * ((N_CTX + BUCKET - 1) // BUCKET)
    seen = set()
    before = _tally(st)

    def check(i, npst, k, lg):
        for r in range(3):
            pos = npst[r] + k - 1
            err = _check_row(lg[r], ref[r][pos], tol, (preset, dt, i, r, pos, k))
            worst[pos // BUCKET] = max(worst[pos // BUCKET], err)
            seen.add(pos)

    _sweep(E, st, seqs, check)
    assert seen >= set(range(3, N_CTX))
    print(f"\n{preset} dtype {dt} worst logit error per position bucket: {_buckets(worst)}  (tol {tol})")
    print(f"  variants: {sorted(_delta(_tally(st), before))}")
    # ohw_decode's position rule at its edge: 440 + 8 = 448 tokens is the whole context, 441 + 8 is past it
    lg = st.decode(np.asarray([s[440:448] for s in seqs], np.int32), [440, 440, 440])
    for r in range(3):
        _check_row(lg[r], ref[r][447], tol, (preset, dt, "edge", r))
    with pytest.raises(E.TranscriptionFailed):
        st.decode(np.asarray([s[440:448] for s in seqs], np.int32), [441, 440, 440])
    with pytest.raises(E.TranscriptionFailed):
        st.decode(np.asarray([s[440:448] for s in seqs], np.int32), [440, 440, 441])
    om.close()


# ---------------------------------------------------------------------------------------------------------------------
# (b) the variant matrix at micro dims (d = 256, 4 heads, n_vocab 51865)
# ---------------------------------------------------------------------------------------------------------------------
# dec_gemm_pick (decode.hip), mt = ceil(M / 16) m-tiles, n_tiles = N / 16: qkv 48, o / xq / xo / fc2 16, fc1 64, logits 3242;
# cus = the stream's CUs (256 on a full-chip stream).
#   LayerNorm GEMMs (qkv, xq, fc1): mt <= 2: 1x1 if n_tiles * mt <= cus, else 2x1 if ceil(n_tiles / 2) * mt <= cus or
#     mt == 1; mt > 2: 4x2 if ceil(n_tiles / 2) * ceil(mt / 2) > 2 * cus, else 2x2 if n_tiles > cus, else 1x2.  mt == 2 with
#     neither fitting falls through to 2x2 as well.
#   RESID GEMMs (o, xo, fc2): 1x1 if mt == 1 or n_tiles * mt <= 2 * cus; else 4x2 if n_tiles * ceil(mt / 2) > 2 * cus; else
#     1x2.  fc2 has K = 4d = 1024 <= DG_LN_MAXK (1280) at micro, so it reaches 4x2 here; at large-v3 (K = 5120) it cannot.
#     2x1 / 2x2 are not reachable for RESID by design (they belong to the LayerNorm and logits rules).
#   logits: mt == 1: 2x1; mt > 2 with 3242 * ceil(mt / 2) > 2 * cus (always at micro): 4x2; else 2x2.  1x1 / 1x2 only with
#     OHW_LOGITS_NT != 2 (not the default path).
# launch_cross_attn: batch_invariant: rows<n> for n_new 2..4, else plain.  Otherwise M <= xa_rows (24) with M * 4 heads < 512
# pairs: split (keys over gridDim.z = 8); more rows: plain.  rows<n> without batch_invariant needs (M / n) * heads >= 256,
# i.e. 64 windows: not reachable at micro with 12.  group*: beam search only (test (d) below).
# (windows B, n_new, CUs of the stream (0: all), batch_invariant) -> the variants the case's calls launch, exactly.
_V = lambda qkv, o, xq, xo, fc1, fc2, lg, xa: frozenset({  # noqa: E731
    f"dec_gemm.qkv.ln.{qkv}", f"dec_gemm.o.{o}", f"dec_gemm.xq.ln.{xq}", f"dec_gemm.xo.{xo}", f"dec_gemm.fc1.ln.{fc1}",
    f"dec_gemm.fc2.{fc2}", f"dec_gemm.logits.{lg}", f"xattn.{xa}", "self_attn.plain"})
VARIANT_CASES = {
    # M = 1 / 16 / 18 / 32: one or two m-tiles on 256 CUs
    (1, 1, 0, False): _V("1x1", "1x1", "1x1", "1x1", "1x1", "1x1", "2x1", "split"),
    (2, 8, 0, False): _V("1x1", "1x1", "1x1", "1x1", "1x1", "1x1", "2x1", "split"),
    (9, 2, 0, False): _V("1x1", "1x1", "1x1", "1x1", "1x1", "1x1", "2x2", "split"),
    (4, 8, 0, False): _V("1x1", "1x1", "1x1", "1x1", "1x1", "1x1", "2x2", "plain"),
    # M = 33 / 96: two-m-tile LayerNorm GEMMs, the logits' 4x2
    (11, 3, 0, False): _V("1x2", "1x1", "1x2", "1x1", "1x2", "1x1", "4x2", "plain"),
    (12, 8, 0, False): _V("1x2", "1x1", "1x2", "1x1", "1x2", "1x1", "4x2", "plain"),
    # a 16-CU stream (a lane of the LANES schedule, narrowed): 2x1 at one m-tile, 2x2 at two, 4x2 from M = 33 (LayerNorm)
    # and M = 65 (RESID); RESID 1x2 at M 33..64
    (1, 1, 16, False): _V("2x1", "1x1", "1x1", "1x1", "2x1", "1x1", "2x1", "split"),
    (3, 6, 16, False): _V("2x2", "1x1", "2x1", "1x1", "2x2", "1x1", "2x2", "split"),
    (11, 3, 16, False): _V("4x2", "1x2", "1x2", "1x2", "4x2", "1x2", "4x2", "plain"),
    (9, 8, 16, False): _V("4x2", "4x2", "1x2", "4x2", "4x2", "4x2", "4x2", "plain"),
    # an 8-CU stream: the xq projection's 2x2 (M 33..64) and 4x2 (M >= 65)
    (6, 8, 8, False): _V("4x2", "4x2", "2x2", "4x2", "4x2", "4x2", "4x2", "plain"),
    (12, 8, 8, False): _V("4x2", "4x2", "4x2", "4x2", "4x2", "4x2", "4x2", "plain"),
    # ohw_state_set_batch_invariant: the cross-attention variant from n_new alone
    (3, 2, 0, True): _V("1x1", "1x1", "1x1", "1x1", "1x1", "1x1", "2x1", "rows2"),
    (3, 3, 0, True): _V("1x1", "1x1", "1x1", "1x1", "1x1", "1x1", "2x1", "rows3"),
    (3, 4, 0, True): _V("1x1", "1x1", "1x1", "1x1", "1x1", "1x1", "2x1", "rows4"),
    (3, 5, 0, True): _V("1x1", "1x1", "1x1", "1x1", "1x1", "1x1", "2x1", "plain"),
}
# every variant of dec_gemm_pick / launch_cross_attn the default path can take at micro dims with up to 96 rows
EXPECTED_VARIANTS = frozenset({
    "dec_gemm.qkv.ln.1x1", "dec_gemm.qkv.ln.2x1", "dec_gemm.qkv.ln.1x2", "dec_gemm.qkv.ln.2x2", "dec_gemm.qkv.ln.4x2",
    "dec_gemm.xq.ln.1x1", "dec_gemm.xq.ln.2x1", "dec_gemm.xq.ln.1x2", "dec_gemm.xq.ln.2x2", "dec_gemm.xq.ln.4x2",
    "dec_gemm.fc1.ln.1x1", "dec_gemm.fc1.ln.2x1", "dec_gemm.fc1.ln.1x2", "dec_gemm.fc1.ln.2x2", "dec_gemm.fc1.ln.4x2",
    "dec_gemm.o.1x1", "dec_gemm.o.1x2", "dec_gemm.o.4x2",
    "dec_gemm.xo.1x1", "dec_gemm.xo.1x2", "dec_gemm.xo.4x2",
    "dec_gemm.fc2.1x1", "dec_gemm.fc2.1x2", "dec_gemm.fc2.4x2",
    "dec_gemm.logits.2x1", "dec_gemm.logits.2x2", "dec_gemm.logits.4x2",
    "xattn.plain", "xattn.split", "xattn.rows2", "xattn.rows3", "xattn.rows4",
    "self_attn.plain",
})
# decode_active: inactive windows skip their cross-attention (the done flags), in the split form and in the plain one
ACTIVE_CASES = {(3, 1, 0, False): [1, 0, 1], (5, 8, 0, False): [0, 1, 1, 0, 1]}


def test_variant_table_covers_the_expected_set():
    assert frozenset().union(*VARIANT_CASES.values()) == EXPECTED_VARIANTS
    for (B, k, _, _), _v in VARIANT_CASES.items():
        assert 1 <= B <= 12 and 1 <= k <= 8


@pytest.mark.parametrize("dt", [0, 1])
def test_every_decoder_variant_matches_the_oracle(E, oracle, tmp_models, dt):
    path = tmp_models("micro")
    om = oracle.Model.load(path)
    ctx = E.Context.from_file(path, 0, dt)
    tol = TOL_LOGIT[dt]
    pcm = np.stack([synth.synth_audio(60 + w) for w in range(12)])
    seqs = [_tokens(ctx.tok, 2000 + w, 80) for w in range(12)]
    refs = {}                                      # (window, encoder output bytes) -> all-position oracle logits

    def ref_of(w, enc):
        key = (w, enc.tobytes())
        if key not in refs:
            s = oracle.State(om)
            s.set_encoder_output(enc)
            refs[key] = s.decode(seqs[w], 0, all_pos=True)
            s.close()
        return refs[key]

    streams = {n: E.Stream(0, 0, n) for n in (8, 16)}
    launched = set()
    worst = 0.0
    for case in list(VARIANT_CASES) + list(ACTIVE_CASES):
        B, k, cus, inv = case
        st = E.State(ctx, 12)
        st.set_batch_invariant(inv)
        st.mel(pcm[:B], None, E.OHW_MEL_ZERO_TAIL, want=False)
        st.encode(B)
        enc = st.fetch("enc", B)
        ref = [ref_of(w, enc[w]) for w in range(B)]
        if cus:
            st.set_stream(streams[cus].ptr)
        # positions 0 .. p0 - 1 in 8-token calls, then the case's calls across the first chunk edge (63|64)
        p0 = 56 if k == 8 else 60
        p = 0
        while p < p0:
            n = min(8, p0 - p)
            lg = st.decode(np.asarray([s[p:p + n] for s in seqs[:B]], np.int32), [p] * B)
            for w in range(B):
                worst = max(worst, _check_row(lg[w], ref[w][p + n - 1], tol, (case, "prefill", w, p)))
            p += n
        before = _tally(st)
        while p + k <= 72:
            lg = st.decode(np.asarray([s[p:p + k] for s in seqs[:B]], np.int32), [p] * B)
            for w in range(B):
                worst = max(worst, _check_row(lg[w], ref[w][p + k - 1], tol, (case, w, p)))
            p += k
        got = _delta(_tally(st), before)
        if case in VARIANT_CASES:
            assert set(got) == VARIANT_CASES[case], (case, sorted(got), sorted(VARIANT_CASES[case]))
        if case in ACTIVE_CASES:
            act = ACTIVE_CASES[case]
            before = _tally(st)
            lg = st.decode_active(np.asarray([s[p:p + k] for s in seqs[:B]], np.int32), [p] * B, act)
            for w in range(B):
                if act[w]:
                    worst = max(worst, _check_row(lg[w], ref[w][p + k - 1], tol, (case, "active", w, p)))
                else:
                    assert not lg[w].any()
            xa = {n for n in _delta(_tally(st), before) if n.startswith("xattn.")}
            assert xa == {"xattn.split" if B * k <= 24 else "xattn.plain"}, (case, xa)
        launched |= set(_tally(st))
        print(f"  case windows={B} n_new={k} cus={cus or 'all'} invariant={inv}: {sorted(got)}")
        st.set_stream(None)
        st.close()
    for s_ in streams.values():
        s_.close()
    print(f"dtype {dt}: worst logit error over the variant matrix {worst:.4f} (tol {tol}); launched {len(launched)} variants")
    assert launched == EXPECTED_VARIANTS, (sorted(launched - EXPECTED_VARIANTS), sorted(EXPECTED_VARIANTS - launched))
    om.close()


# ---------------------------------------------------------------------------------------------------------------------
# (c) large-v3 dims (the bench's model): one window, teacher-forced 0 .. 447, and a greedy walk of 110 steps
# ---------------------------------------------------------------------------------------------------------------------
def test_large_v3_dims_at_every_depth(E, oracle):
    """K = d = 1280 = DG_LN_MAXK (the fused-LayerNorm limit), the logits GEMM at n_tiles > CUs; bf16 and f16"""
    hp = synth.PRESETS["large-v3"]
    om = oracle.Model.synth(hp.as_list(), 1234)
    pcm = synth.synth_audio(0)[None]
    t_oracle = 0.0
    for dt in (0, 1):
        ctx = E.Context.synthetic(hp.as_list(), 1234, 0, dt)
        st = E.State(ctx, 1)
        st.mel(pcm, None, E.OHW_MEL_ZERO_TAIL, want=False)
        st.encode(1)
        enc = st.fetch("enc", 1)[0]
        seq = _tokens(ctx.tok, 3000)
        t0 = time.time()
        s = oracle.State(om)
        s.set_encoder_output(enc)
        ref = s.decode(seq, 0, all_pos=True)
        t_oracle += time.time() - t0
        worst = [0.0] * ((N_CTX + BUCKET - 1) // BUCKET)
        worst_sig = 0.0
        lg = st.decode(np.asarray([seq[:4]], np.int32), [0])[0]
        for pos in range(3, N_CTX):
            if pos >= 4:
                lg = st.decode(np.asarray([[seq[pos]]], np.int32), [pos])[0]
            sig = float(ref[pos].std())
            err = float(np.abs(lg - ref[pos]).max())
            worst[pos // BUCKET] = max(worst[pos // BUCKET], err)
            worst_sig = max(worst_sig, err / sig)
            assert err < 0.07 * sig, (dt, pos, err, sig)
            if int(lg.argmax()) != int(ref[pos].argmax()):
                top = np.sort(ref[pos])[-2:]
                assert top[1] - top[0] < 0.14 * sig, (dt, pos)
        print(f"\nlarge-v3 dtype {dt} worst logit error per position bucket: {_buckets(worst)}  (worst {worst_sig:.4f} sigma, tol 0.07)")
        if dt == 0:
            # the device greedy loop for 110 steps with config #5's timestamp bias (tests/test_gpu_configs.py); the oracle
            # walks the GPU's path and must pick the same token, except where its own top-2 margin is a near-tie.  The
            # procedural weights' logits barely depend on the context: an unbiased walk repeats one token, this one visits 3
            # (observed; static biases that flatten 48 or 512 text tokens settle into a 2-cycle).  The cache at depth is
            # carried by the teacher-forced sweep above, whose 448 positions each see another token.
            bias = np.zeros(om.n_vocab, np.float32)
            bias[om.tok_beg:] = 4.0
            bias[om.tok_eot] = 9.0
            p = ctx.default_params()
            p.force_len = 110
            st.set_logit_bias(bias)
            dev = st.greedy_ex(1, p)[0]
            assert len(dev["tokens"]) == 110
            distinct = len(set(dev["tokens"]))
            op = om.default_params()
            op.force_len = 110
            t0 = time.time()
            walk = s.greedy_ex(op, bias, dev["tokens"])
            t_oracle += time.time() - t0
            sig = float(ref[3].std())
            same = 0
            for i, t in enumerate(dev["tokens"]):
                if walk["choice"][i] == t:
                    same += 1
                else:
                    assert walk["margins"][i] < 0.14 * sig, (i, t, walk["choice"][i], float(walk["margins"][i]))
            print(f"large-v3 greedy walk: oracle picks the GPU's token {same} / {len(dev['tokens'])}, {distinct} distinct tokens")
            assert distinct >= 3
            assert same >= 0.9 * len(dev["tokens"])
        s.close()
        st.close()
        ctx.close()                               # ~3 GB: freed before the next dtype's context
    print(f"large-v3 oracle time: {t_oracle:.1f} s")
    om.close()


# ---------------------------------------------------------------------------------------------------------------------
# (d) beam search past one slot chunk: the kv_slot self-attention over more than 64 keys
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [1, 0])
def test_beam_search_past_one_slot_chunk(E, oracle, tmp_models, dt):
    """n_max 110 with end-of-text disfavoured: the beams live to position 113, the slot tables span two chunks.  Two windows
    (10 rows: the beams' split cross-attention) and five (25 rows, past xa_rows: cross_attn_rows_kernel<5>).  The rule of
    tests/test_gpu_beam.py: the oracle's exact winner, or a sequence that scores as well under the oracle."""
    path = tmp_models("micro")
    om = oracle.Model.load(path)
    ctx = E.Context.from_file(path, 0, dt)
    K, n_max = 5, 110
    bias = np.zeros(om.n_vocab, np.float32)
    bias[om.tok_beg:] = 4.0
    bias[om.tok_eot] = -30.0
    p = ctx.default_params(); p.n_max = n_max
    op = om.default_params(); op.n_max = n_max
    exact = total = 0
    for W, want in ((2, {"xattn.group_split", "self_attn.slots"}), (5, {"xattn.group5", "self_attn.slots"})):
        st = E.State(ctx, W * K)
        st.set_logit_bias(bias)
        st.mel(np.stack([synth.synth_audio(80 + w) for w in range(W)]), None, E.OHW_MEL_ZERO_TAIL, want=False)
        st.encode(W)
        enc = st.fetch("enc", W)
        got = st.beam_search(W, K, p)
        tally = _tally(st)
        assert want <= set(tally), (W, sorted(tally))
        for w in range(W):
            g = got[w]
            assert len(g["tokens"]) > 64, (w, len(g["tokens"]))
            ref = oracle.beam_search(om, enc[w], op, K, bias)
            total += 1
            if g["tokens"] == ref["tokens"]:
                exact += 1
                assert abs(g["sum_logprob"] - ref["sum_logprob"]) < (0.5 if dt == 0 else 0.06) * max(1, len(g["tokens"])) ** 0.5
            else:
                s = oracle.State(om)
                s.set_encoder_output(enc[w])
                best = max(c[1] / max(1, len(c[0])) for c in ref["candidates"])
                mine = max(s.score_sequence(op, g["tokens"], e, bias) / max(1, len(g["tokens"])) for e in (True, False))
                s.close()
                assert mine > best - (0.1 if dt == 0 else 0.02), (W, w, mine, best)
        st.close()
    print(f"\nbeam search past 64 positions: {exact} / {total} windows with the oracle's exact winner (dtype {dt})")
    om.close()


# ---------------------------------------------------------------------------------------------------------------------
# (e) the opt-in variants at depth, against the launch path (no oracle)
# ---------------------------------------------------------------------------------------------------------------------
def _sweep_logits(E, st, seqs):
    out = []
    _sweep(E, st, seqs, lambda i, npst, k, lg: out.append(lg))
    return out


def test_fused_self_attention_at_every_depth(E, oracle, tmp_models, monkeypatch):
    """OHW_DEC_FUSE_ATTN=1: the separate launch's bits at every position of the sweep"""
    monkeypatch.setenv("OHW_DEC_FUSE_ATTN", "1")
    _, ctx, fused, seqs = _depth_setup(E, oracle, tmp_models, "micro", 1)
    monkeypatch.setenv("OHW_DEC_FUSE_ATTN", "0")
    plain = E.State(ctx, 3)
    plain.mel(np.stack([synth.synth_audio(40 + r) for r in range(3)]), None, E.OHW_MEL_ZERO_TAIL, want=False)
    plain.encode(3)
    a, b = _sweep_logits(E, fused, seqs), _sweep_logits(E, plain, seqs)
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), (i, float(np.abs(x - y).max()))
    assert fused.counter("self_attn.fused") > 0 and plain.counter("self_attn.fused") == 0


def test_persistent_step_at_every_depth(E, oracle, tmp_models):
    """ohw_state_set_persistent: the launch path's logits within the f16 logit tolerance at every position of the sweep"""
    _, ctx, pers, seqs = _depth_setup(E, oracle, tmp_models, "micro", 1)
    pers.set_persistent(True)
    plain = E.State(ctx, 3)
    plain.mel(np.stack([synth.synth_audio(40 + r) for r in range(3)]), None, E.OHW_MEL_ZERO_TAIL, want=False)
    plain.encode(3)
    a, b = _sweep_logits(E, pers, seqs), _sweep_logits(E, plain, seqs)
    worst = max(float(np.abs(x - y).max()) for x, y in zip(a, b))
    print(f"\npersistent step vs launch path over the sweep: worst {worst:.4f}")
    assert worst < TOL_LOGIT[1]
    assert pers.counter("persist_launches") > 0 and plain.counter("persist_launches") == 0
