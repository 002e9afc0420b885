"""Reduced audio context (ohw_state_set_audio_ctx, whisper.cpp's audio_ctx) on the GPU against the CPU oracle.

The oracle is always oracle.Model.synth with n_audio_ctx = C (tests/test_audio_ctx_cpu.py: the full model with the first C
positional rows).  It is fed the GPU's own fetched log-mel with the frames from 2C on zeroed - frame 2C is conv1's padding -
and, for the decoder checks, the GPU's own encoder output (as tests/test_gpu_decoder_depth.py does).

Tolerances are those of tests/test_gpu_parity.py and DESIGN.md section 3, unchanged:
  micro dims     activations bf16 6e-2 / f16 8e-3 (twice that after a block and on encoder output / cross K/V), logits 0.25 / 0.03
  large-v3 dims  encoder output 0.07 max and 0.011 mean, logits 0.07 sigma
  greedy picks   the oracle's token, or the oracle's own top-2 margin is inside twice the logit tolerance
The short-window GEMM (ohw_dbg_gemm_small) takes the bounds tests/test_gpu_kernels.py applies to ohw_dbg_gemm.
"""
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

from openhush_amd import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_ACT = {0: 6e-2, 1: 8e-3}
TOL_LOGIT = {0: 0.25, 1: 0.03}
MICRO = synth.PRESETS["micro"]


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
    return o


@pytest.fixture(scope="module")
def ctxs(E):
    return {dt: E.Context.synthetic(MICRO.as_list(), 1234, 0, dt) for dt in (0, 1)}


@pytest.fixture(scope="module")
def omodel(oracle):
    cache = {}

    def get(C, hp=MICRO):
        key = (C, hp.n_audio_state)
        if key not in cache:
            hl = hp.as_list()
            hl[1] = C
            cache[key] = oracle.Model.synth(hl, 1234)
        return cache[key]
    yield get
    for m in cache.values():
        m.close()


def _pcm_batch():
    a = synth.synth_audio(7)
    b = np.zeros(synth.CHUNK_SAMPLES, np.float32)
    b[:48000] = synth.synth_audio(3, 48000)
    c = synth.synth_audio(11)
    return np.stack([a, b, c]), [synth.CHUNK_SAMPLES, 48000, synth.CHUNK_SAMPLES]


def _cut(mel, C):
    z = mel.copy()
    z[:, 2 * C:] = 0
    return z


def _front(E, ctx, C, B=3, max_batch=None):
    pcm, ns = _pcm_batch()
    st = E.State(ctx, max_batch or B)
    st.set_audio_ctx(C)
    mel = st.mel(pcm[:B], ns[:B], E.OHW_MEL_ZERO_TAIL)
    st.encode(B)
    return st, mel


def _oracle_states(oracle, om, enc):
    out = []
    for b in range(enc.shape[0]):
        s = oracle.State(om)
        s.set_encoder_output(enc[b])
        out.append(s)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# encoder
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C", [8, 63, 250, 256, 750, 1499])
def test_encoder_matches_reduced_context_oracle(E, oracle, ctxs, omodel, dt, B, C):
    om = omodel(C)
    st, mel = _front(E, ctxs[dt], C, B)
    assert st.audio_ctx == C
    pcm, ns = _pcm_batch()
    tol = TOL_ACT[dt]
    stem, block0, enc = (st.fetch(k, B) for k in ("stem", "block0", "enc"))
    L = ctxs[dt].hp.n_text_layer
    xk0, xvl = st.fetch("xk0", B), st.fetch(f"xv{L - 1}", B)
    assert stem.shape == (B, C, MICRO.n_audio_state) and xk0.shape == (B, C, MICRO.n_text_state)
    worst = {}
    for b in range(B):
        assert np.abs(mel[b] - om.log_mel(pcm[b, :ns[b]], 1)).max() < 2e-4          # the log-mel itself does not change
        r_enc, _, r_stem, r_b0 = om.encode(_cut(mel[b], C), taps=True)
        s = oracle.State(om)
        s.set_encoder_output(enc[b])                                                # the GPU's own encoder output
        k, v = s.cross_kv()
        for name, got, ref, t in (("stem", stem[b], r_stem, tol), ("block0", block0[b], r_b0, 2 * tol), ("enc", enc[b], r_enc, 2 * tol),
                                  ("xk0", xk0[b], k[0], 2 * tol), ("xvl", xvl[b], v[L - 1], 2 * tol)):
            err = float(np.abs(got - ref).max())
            worst[name] = max(worst.get(name, 0.0), err)
            assert err < t, (name, b, err, t)
    print(f"\naudio_ctx {C} B {B} dtype {dt}: worst abs err {({k: round(v, 5) for k, v in worst.items()})}")


def test_large_v3_dims_reduced_context_matches_oracle(E, oracle, omodel):
    """large-v3 dims, C = 256 (a 5 s chunk's neighbourhood), bf16 and f16: encoder output against the oracle, then the
    prompt's and three more steps' logits against an oracle decoder fed the GPU's own encoder output."""
    hp = synth.PRESETS["large-v3"]
    C = 256
    oracle.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    om = omodel(C, hp)
    pcm = synth.synth_audio(0)[None]
    for dt in (0, 1):
        ctx = E.Context.synthetic(hp.as_list(), 1234, 0, dt)
        st = E.State(ctx, 1)
        st.set_audio_ctx(C)
        mel = st.mel(pcm, None, E.OHW_MEL_ZERO_TAIL)
        st.encode(1)
        enc = st.fetch("enc", 1)[0]
        assert enc.shape == (C, hp.n_audio_state)
        err = np.abs(enc - om.encode(_cut(mel[0], C)))
        print(f"\nlarge-v3 audio_ctx {C} dtype {dt}: encoder output max abs err {err.max():.4f}, mean {err.mean():.5f}")
        assert err.max() < 0.07 and err.mean() < 0.011, (dt, err.max(), err.mean())
        s = oracle.State(om)
        s.set_encoder_output(enc)
        prompt = [ctx.tok.sot, ctx.tok.sot + 1, ctx.tok.transcribe]
        ref = s.decode(prompt, 0)
        got = st.decode(np.asarray([prompt], np.int32), [0])[0]
        sig = float(ref.std())
        worst = float(np.abs(got - ref).max())
        assert worst < 0.07 * sig, (dt, worst, sig)
        tok = int(ref.argmax())
        for i in range(3):
            ref = s.decode([tok], 3 + i)
            got = st.decode(np.asarray([[tok]], np.int32), [3 + i])[0]
            worst = max(worst, float(np.abs(got - ref).max()))
            assert np.abs(got - ref).max() < 0.07 * sig, (dt, i)
            tok = int(ref.argmax())
        print(f"large-v3 audio_ctx {C} dtype {dt}: worst logit err {worst:.4f} at sigma {sig:.3f} ({worst / sig:.4f} sigma)")
        st.close()
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------
# decoder, every cross-attention variant at a reduced context
# ---------------------------------------------------------------------------------------------------------------------------
def _forced(ctx, n=14):
    rng = np.random.default_rng(5)
    return [ctx.tok.sot, ctx.tok.sot + 1, ctx.tok.transcribe, ctx.tok.timestamp_begin] + [int(t) for t in rng.integers(1000, 30000, n - 4)]


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("C,invariant", [(250, False), (250, True), (63, False), (750, False)])
def test_teacher_forced_logits_at_reduced_context(E, oracle, ctxs, omodel, dt, C, invariant):
    """3 windows: the prompt's 4 tokens in one call (plain / split per row, or rows4 under batch-invariant mode), then one
    token per call; C = 250 is no multiple of the 8-key group, 63 is shorter than one key slice, 250 and 750 are split."""
    om = omodel(C)
    ctx = ctxs[dt]
    st, _ = _front(E, ctx, C)
    st.set_batch_invariant(invariant)
    enc = st.fetch("enc", 3)
    ost = _oracle_states(oracle, om, enc)
    forced = _forced(ctx)
    ref_all = [s.decode(forced, 0, all_pos=True) for s in ost]
    tol = TOL_LOGIT[dt]
    lg = st.decode(np.tile(np.asarray(forced[:4], np.int32), (3, 1)), [0, 0, 0])
    worst = max(float(np.abs(lg[b] - ref_all[b][3]).max()) for b in range(3))
    for i in range(4, len(forced)):
        lg = st.decode(np.full((3, 1), forced[i], np.int32), [i, i, i])
        for b in range(3):
            worst = max(worst, float(np.abs(lg[b] - ref_all[b][i]).max()))
    print(f"\naudio_ctx {C} invariant {invariant} dtype {dt}: worst logit err {worst:.4f} (tol {tol})")
    assert worst < tol, worst
    if invariant:
        assert st.counter("xattn.rows4") > 0 and st.counter("xattn.plain") > 0 and st.counter("xattn.split") == 0
    elif C >= 128:
        assert st.counter("xattn.split") > 0 and st.counter("xattn.plain") == 0
    else:
        assert st.counter("xattn.plain") > 0 and st.counter("xattn.split") == 0      # 63 keys: no slice of 64
    # decode_active: the inactive window is skipped, the others keep their bits
    i = len(forced)
    full = st.decode(np.full((3, 1), 1234, np.int32), [i, i, i])
    part = st.decode_active(np.full((3, 1), 1234, np.int32), [i, i, i], [1, 0, 1])
    assert np.array_equal(part[0], full[0]) and np.array_equal(part[2], full[2]) and not part[1].any()


def _check_greedy(oracle, om, enc_b, dev_b, n_max, tol):
    s = oracle.State(om)
    s.set_encoder_output(enc_b)
    op = om.default_params()
    op.n_max = n_max
    forced = dev_b["tokens"] + ([om.tok_eot] if dev_b["ended_by_eot"] else [])
    ref = s.greedy_ex(op, None, forced)
    same = 0
    for i, t in enumerate(forced):
        if ref["choice"][i] == t:
            same += 1
        else:
            assert ref["margins"][i] < 2 * tol, (i, t, ref["choice"][i], float(ref["margins"][i]))
    return same, len(forced)


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("mode", ["plain", "invariant", "persist", "fused"])
def test_greedy_walk_at_reduced_context(E, oracle, ctxs, omodel, dt, mode, monkeypatch):
    """greedy_ex (the captured step graph) at C = 250 on 3 windows: the launches, batch-invariant mode, the persistent step and
    self-attention fused into the QKV launch; every pick is judged by the oracle's top-2 margin."""
    C = 250
    om = omodel(C)
    ctx = ctxs[dt]
    if mode == "fused":
        monkeypatch.setenv("OHW_DEC_FUSE_ATTN", "1")
    st, _ = _front(E, ctx, C)
    if mode == "invariant":
        st.set_batch_invariant(True)
    if mode == "persist":
        st.set_persistent(True)
    enc = st.fetch("enc", 3)
    p = ctx.default_params()
    p.n_max = 32
    dev = st.greedy_ex(3, p)
    assert st.greedy_ex(3, p)[0]["tokens"] == dev[0]["tokens"]
    same = total = 0
    for b in range(3):
        a, n = _check_greedy(oracle, om, enc[b], dev[b], 32, TOL_LOGIT[dt])
        same += a
        total += n
    print(f"\naudio_ctx {C} {mode} dtype {dt}: oracle picks the GPU's token {same} / {total}")
    assert same >= 0.9 * total
    if mode == "persist":
        assert st.counter("persist_launches") > 0
    if mode == "fused":
        assert st.counter("self_attn.fused") > 0
    if mode == "plain":
        assert st.greedy(3, p)[0] == [d["tokens"] for d in dev]      # ohw_greedy: the same loop


@pytest.mark.parametrize("dt", [1, 0])
def test_beam_sample_pass_and_language_at_reduced_context(E, oracle, ctxs, omodel, dt):
    C = 250
    om = omodel(C)
    ctx = ctxs[dt]
    K = 5
    bias = np.zeros(om.n_vocab, np.float32)
    bias[om.tok_beg:] = 6.0
    bias[om.tok_eot] = 27.0
    p = ctx.default_params()
    p.n_max = 24
    op = om.default_params()
    op.n_max = 24
    for invariant in (False, True):        # group_split (few windows: keys cut), then group5 (one workgroup per window and head)
        st, _ = _front(E, ctx, C, 3, 3 * K)
        st.set_batch_invariant(invariant)
        st.set_logit_bias(bias)
        enc = st.fetch("enc", 3)
        got = st.beam_search(3, K, p)
        assert st.beam_search(3, K, p) == got
        assert st.counter("xattn.group5" if invariant else "xattn.group_split") > 0
        for w in range(3):
            ref = oracle.beam_search(om, enc[w], op, K, bias)
            g = got[w]
            assert len(g["tokens"]) > 0
            if g["tokens"] != ref["tokens"]:
                s = oracle.State(om)
                s.set_encoder_output(enc[w])
                best = max(c[1] / max(1, len(c[0])) for c in ref["candidates"])
                mine = max(s.score_sequence(op, g["tokens"], e, bias) / max(1, len(g["tokens"])) for e in (True, False))
                assert mine > best - (0.1 if dt == 0 else 0.02), (invariant, w, g, ref["tokens"], mine, best)
    # one rung of the temperature ladder on the device: window 1 rides along inactive; picks are draws, so the check is that
    # every sampled token has the log-probability the oracle gives it at that temperature on the same path
    st, _ = _front(E, ctx, C)
    enc = st.fetch("enc", 3)
    cap = ctx.hp.n_text_ctx
    u = np.random.default_rng(3).random((3, cap))
    p2 = ctx.default_params()
    p2.n_max = 16
    res = st.sample_pass(3, 0.4, [1, 0, 1], u, p2)
    assert res[1]["tokens"] == [] and len(res[0]["tokens"]) > 0 and len(res[2]["tokens"]) > 0
    assert st.sample_pass(3, 0.4, [1, 0, 1], u, p2)[0]["tokens"] == res[0]["tokens"]
    op2 = om.default_params()
    op2.n_max = 16
    for b in (0, 2):
        s = oracle.State(om)
        s.set_encoder_output(enc[b])
        forced = res[b]["tokens"] + ([om.tok_eot] if res[b]["ended_by_eot"] else [])
        r = s.decode_pass(op2, None, 0.4, oracle.MT19937(0), forced)
        for i in range(len(res[b]["tokens"])):
            assert abs(float(r["plogs"][i]) - float(res[b]["logprobs"][i])) < 2 * TOL_LOGIT[dt] / 0.4, (b, i)
    # language detection runs one decoder step under the reduced context
    ids, probs = st.detect_language(3)
    for b in range(3):
        s = oracle.State(om)
        s.set_encoder_output(enc[b])
        lg = s.decode([om.tok_sot], 0)
        lang = lg[om.tok_sot + 1: om.tok_sot + 1 + probs.shape[1]]
        top2 = np.sort(lang)[-2:]
        assert int(ids[b]) == int(lang.argmax()) or top2[1] - top2[0] < 2 * TOL_LOGIT[dt]
        assert abs(float(probs[b].sum()) - 1.0) < 1e-3


def test_every_cross_attention_variant_ran_at_a_reduced_context(E, ctxs):
    """one state, C = 256: plain, split, rows2..4, group2..5 and group_split are each launched with 256 keys"""
    ctx = ctxs[1]
    st, _ = _front(E, ctx, 256, 3, 15)
    toks = lambda n: np.full((3, n), 2000, np.int32)       # noqa: E731
    st.decode(toks(1), [0, 0, 0])                                                       # 3 rows: split
    assert st.counter("xattn.split") > 0
    st.set_batch_invariant(True)
    for n in (1, 2, 3, 4):
        st.decode(toks(n), [0, 0, 0])                                                   # plain, rows2, rows3, rows4
    p = ctx.default_params()
    p.n_max = 6
    for K in (2, 3, 4, 5):
        st.beam_search(3, K, p)                                                         # group2 .. group5
    st.set_batch_invariant(False)
    st.beam_search(3, 2, p)                                                             # 3 windows x 2 beams: group_split
    for name in ("plain", "split", "rows2", "rows3", "rows4", "group2", "group3", "group4", "group5", "group_split"):
        assert st.counter("xattn." + name) > 0, name


# ---------------------------------------------------------------------------------------------------------------------------
# switching contexts on one state, slices, bad values
# ---------------------------------------------------------------------------------------------------------------------------
def _greedy_run(E, st, C, n_max=24):
    pcm, ns = _pcm_batch()
    st.set_audio_ctx(C)
    st.mel(pcm[:2], ns[:2], E.OHW_MEL_ZERO_TAIL, want=False)
    st.encode(2)
    lg = st.decode(np.tile(np.asarray([st.ctx.tok.sot, st.ctx.tok.sot + 1, st.ctx.tok.transcribe], np.int32), (2, 1)), [0, 0])
    p = st.ctx.default_params()
    p.n_max = n_max
    return lg, st.greedy_ex(2, p)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and all(x["tokens"] == y["tokens"] and np.array_equal(x["logprobs"], y["logprobs"]) for x, y in zip(a[1], b[1]))


@pytest.mark.parametrize("dt", [0, 1])
def test_switching_contexts_is_bit_equal_to_fresh_states(E, ctxs, dt):
    ctx = ctxs[dt]
    fresh = {}
    for C in (0, 256):
        s = E.State(ctx, 2)
        fresh[C] = _greedy_run(E, s, C)
        s.close()
    st = E.State(ctx, 2)
    caps = [st.counter("step_captures")]
    for C in (0, 256, 0, 0):
        assert _same(_greedy_run(E, st, C), fresh[C]), C
        caps.append(st.counter("step_captures"))
    assert caps[1] > caps[0] and caps[2] > caps[1]        # a new context is a new graph: t_len is a captured argument
    assert caps[3] == caps[2] and caps[4] == caps[3]      # back at a context already captured: no new capture
    # set_audio_ctx(n_audio_ctx) and set_audio_ctx(0) are the default state
    assert _same(_greedy_run(E, st, ctx.hp.n_audio_ctx), fresh[0]) and st.audio_ctx == ctx.hp.n_audio_ctx
    assert st.counter("step_captures") == caps[4]
    assert fresh[0][1][0]["tokens"] != fresh[256][1][0]["tokens"] or not np.array_equal(fresh[0][0], fresh[256][0])


def test_encode_slices_under_a_reduced_context(E, ctxs):
    ctx = ctxs[0]
    pcm, ns = _pcm_batch()
    C = 250
    one = E.State(ctx, 3)
    one.set_audio_ctx(C)
    one.mel(pcm, ns, E.OHW_MEL_ZERO_TAIL, want=False)
    one.encode(3)
    two = E.State(ctx, 3)
    two.set_audio_ctx(C)
    two.mel(pcm[:2], ns[:2], E.OHW_MEL_ZERO_TAIL, want=False)
    two.encode_slice(2, 0, 3)
    two.mel(pcm[2:], ns[2:], E.OHW_MEL_ZERO_TAIL, want=False)
    two.encode_slice(1, 2, 3)
    L = ctx.hp.n_text_layer
    for what in ("xk0", f"xv{L - 1}"):
        assert np.array_equal(one.fetch(what, 3), two.fetch(what, 3)), what
    t = np.tile(np.asarray([ctx.tok.sot, ctx.tok.sot + 1, ctx.tok.transcribe], np.int32), (3, 1))
    assert np.array_equal(one.decode(t, [0, 0, 0]), two.decode(t, [0, 0, 0]))
    # a later slice under another context than the first is refused
    two.set_audio_ctx(128)
    two.mel(pcm[2:], ns[2:], E.OHW_MEL_ZERO_TAIL, want=False)
    with pytest.raises(E.WhisperError) as ex:
        two.encode_slice(1, 2, 3)
    assert ex.value.code == E.OHW_E_INVALID_ARG


def test_context_mismatch_and_bad_values_are_refused(E, ctxs):
    ctx = ctxs[0]
    st, _ = _front(E, ctx, 256, 1, 5)
    for bad in (-1, ctx.hp.n_audio_ctx + 1, 100000):
        assert E.lib().ohw_state_set_audio_ctx(st.h, bad) == E.OHW_E_INVALID_ARG
    assert st.audio_ctx == 256
    st.set_audio_ctx(128)                                  # no re-encode: every decode entry must refuse, not read stale K/V
    p = ctx.default_params()
    p.n_max = 4
    calls = (lambda: st.decode(np.asarray([[ctx.tok.sot]], np.int32), [0]), lambda: st.decode_active(np.asarray([[ctx.tok.sot]], np.int32), [0], [1]),
             lambda: st.greedy(1, p), lambda: st.greedy_ex(1, p), lambda: st.beam_search(1, 5, p), lambda: st.detect_language(1),
             lambda: st.sample_pass(1, 0.5, [1], np.zeros((1, ctx.hp.n_text_ctx)), p), lambda: st.encode(1))
    for f in calls:
        with pytest.raises(E.WhisperError) as ex:
            f()
        assert ex.value.code == E.OHW_E_INVALID_ARG
    st.set_audio_ctx(256)
    st.decode(np.asarray([[ctx.tok.sot]], np.int32), [0])   # back at the encode's context: fine again


# ---------------------------------------------------------------------------------------------------------------------------
# the short-window GEMM
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("N,K", [(256, 256), (768, 256), (1024, 256), (256, 1024), (256, 384), (1280, 1280), (3840, 1280), (5120, 1280), (1280, 5120)])
@pytest.mark.parametrize("M", [8, 250, 256, 640])
def test_gemm_small_epilogues(E, dt, M, N, K):
    """ohw_dbg_gemm_small on the shapes the encoder gives it (QKV, attn.out, mlp.0, mlp.2, conv1 at micro and large-v3 dims)
    against torch fp32, with the bounds of tests/test_gpu_kernels.py; guard rows behind row M - 1 stay untouched; and it gives
    ohw_dbg_gemm's bits (the same accumulation order per element)."""
    g = torch.Generator(device="cuda").manual_seed(M * 7 + N + K)
    td = torch.bfloat16 if dt == E.OHW_DTYPE_BF16 else torch.float16
    A = (torch.randn(M, K, device="cuda", generator=g) * 0.5).to(td)
    W = (torch.randn(N, K, device="cuda", generator=g) / K ** 0.5).to(td)
    bias = torch.randn(N, device="cuda", generator=g)
    ref = A.float() @ W.float().T + bias
    s = torch.cuda.current_stream().cuda_stream
    L = E.lib()
    out = torch.zeros(M, N, device="cuda")
    assert L.ohw_dbg_gemm_small(dt, A.data_ptr(), W.data_ptr(), bias.data_ptr(), out.data_ptr(), M, N, K, E.EPI_F32, s) == 0, E.last_error()
    torch.cuda.synchronize()
    assert (out - ref).abs().max().item() < 2e-3 * max(1.0, ref.abs().max().item())
    if N % 128 == 0:
        big = torch.zeros(M, N, device="cuda")
        assert L.ohw_dbg_gemm(dt, A.data_ptr(), W.data_ptr(), bias.data_ptr(), big.data_ptr(), M, N, K, E.EPI_F32, s) == 0, E.last_error()
        torch.cuda.synchronize()
        assert torch.equal(big, out)
    for epi, fn in ((E.EPI_BIAS_T, lambda x: x), (E.EPI_BIAS_GELU_T, lambda x: torch.nn.functional.gelu(x))):
        o16 = torch.zeros(M + 3, N, device="cuda", dtype=td)
        assert L.ohw_dbg_gemm_small(dt, A.data_ptr(), W.data_ptr(), bias.data_ptr(), o16.data_ptr(), M, N, K, epi, s) == 0, E.last_error()
        torch.cuda.synchronize()
        want = fn(ref)
        tol = (2 ** -7 if dt == 0 else 2 ** -10) * max(1.0, want.abs().max().item())
        assert (o16[:M].float() - want).abs().max().item() <= tol
        assert not o16[M:].any()
    res = torch.randn(M + 3, N, device="cuda", generator=g)
    acc = res.clone()
    assert L.ohw_dbg_gemm_small(dt, A.data_ptr(), W.data_ptr(), bias.data_ptr(), acc.data_ptr(), M, N, K, E.EPI_BIAS_RESID_F32, s) == 0
    torch.cuda.synchronize()
    assert (acc[:M] - (res[:M] + ref)).abs().max().item() < 2e-3 * max(1.0, ref.abs().max().item())
    assert torch.equal(acc[M:], res[M:])


def test_gemm_small_knob_changes_no_bits(E, ctxs, monkeypatch):
    """OHW_GEMM_SMALL=0 / 1 (conv1, conv2 with positions, the blocks, the cross-K/V epilogue) give the same encoder bits"""
    got = {}
    for knob in ("0", "1"):
        monkeypatch.setenv("OHW_GEMM_SMALL", knob)
        st, _ = _front(E, ctxs[0], 250, 3)
        got[knob] = [st.fetch(k, 3) for k in ("stem", "enc", "xk0", "xv1")]
        st.close()
    for a, b in zip(got["0"], got["1"]):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------------
# engine, pool, streaming session, CLI
# ---------------------------------------------------------------------------------------------------------------------------
def test_engine_pool_session_and_cli_under_audio_ctx(E, tmp_models, tmp_path):
    from openhush_amd import cli, streaming as S
    path = tmp_models("micro")
    clip = synth.synth_audio(5, 80000)                     # 5 s
    C = E.audio_ctx_for(len(clip))
    assert C == 320

    def run(eng, pcm):
        res = eng.transcribe(E.AudioBuffer(pcm.copy(), 16000))
        return res.text, eng.last_tokens()

    eng = E.WhisperEngine.new(path, "auto", False, True, 0, E.OHW_DTYPE_F16, 2)
    eng.set_decode_policy(temperature_inc=0.0)             # T = 0 only: the tokens are the greedy walk's, cut by the acceptance rules
    off = run(eng, clip)
    eng.set_audio_ctx("auto")
    auto = run(eng, clip)
    assert E.lib().ohw_state_audio_ctx(E.lib().ohw_engine_state(eng.h)) == C
    eng.set_audio_ctx(C)
    fixed = run(eng, clip)
    assert auto == fixed and len(auto[1]) > 0
    # the low-level path at ohw_audio_ctx_for(80000): the engine keeps a prefix of that greedy walk (its acceptance rules cut, never add)
    ctx = E.Context.from_file(path, 0, E.OHW_DTYPE_F16)
    st = E.State(ctx, 1)
    st.set_audio_ctx(C)
    st.mel(clip[None, :], [len(clip)], E.OHW_MEL_ZERO_TAIL, want=False)
    st.encode(1)
    low = st.greedy(1)[0][0]
    assert auto[1] == low[:len(auto[1])], (auto[1], low)
    st.set_audio_ctx(0)
    st.mel(clip[None, :], [len(clip)], E.OHW_MEL_ZERO_TAIL, want=False)
    st.encode(1)
    assert off[1] == st.greedy(1)[0][0][:len(off[1])]
    # a fixed context that does not cover the audio fails loudly and names the window
    eng.set_audio_ctx(128)
    with pytest.raises(E.WhisperError) as ex:
        run(eng, clip)
    assert ex.value.code == E.OHW_E_INVALID_ARG and "window 0" in str(ex.value) and "128" in str(ex.value)
    long = np.concatenate([synth.synth_audio(21), synth.synth_audio(22), synth.synth_audio(23, 160000)])       # 70 s
    eng.set_audio_ctx(1400)
    with pytest.raises(E.WhisperError) as ex:
        run(eng, long)
    assert "window 0" in str(ex.value)
    for bad in (-2, 1501):
        assert E.lib().ohw_engine_set_audio_ctx(eng.h, bad) == E.OHW_E_INVALID_ARG
    # 70 s under auto = context off, token for token
    eng.set_audio_ctx(0)
    long_off = run(eng, long)
    eng.set_audio_ctx("auto")
    assert run(eng, long) == long_off and len(long_off[1]) > 0
    assert run(eng, clip) == auto                          # and back to the short clip
    eng.close()
    # the pool (device 0 listed twice)
    pool = E.EnginePool(path, "auto", False, [0, 0], E.OHW_DTYPE_F16, 2)
    pool.set_decode_policy(temperature_inc=0.0)
    pool.set_audio_ctx("auto")
    res = pool.transcribe(E.AudioBuffer(clip.copy(), 16000))
    assert (res.text, pool.last_tokens()) == auto
    res = pool.transcribe(E.AudioBuffer(long.copy(), 16000))
    assert (res.text, pool.last_tokens()) == long_off
    pool.close()
    # the streaming session: greedy over the chunk under the auto context = the low-level walk
    ses = S.StreamingSession(ctx, beam_size=0, audio_ctx="auto")
    out = ses.tick(clip, len(clip), is_final=True)
    assert ses.state.audio_ctx == C
    assert out[0].text == b"".join(ctx.token_text(t) for t in low if t < ctx.tok.eot).decode("utf-8", "replace").strip()
    with pytest.raises(E.WhisperError):
        S.StreamingSession(ctx, beam_size=0, audio_ctx=128).tick(clip, len(clip), is_final=True)
    # the CLI flag
    wav = str(tmp_path / "five.wav")
    with wave.open(wav, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes(np.round(clip * 32767).astype("<i2").tobytes())
    eng = E.WhisperEngine.new(path, "auto", False, True, 0, E.OHW_DTYPE_AUTO, 8)
    eng.set_audio_ctx("auto")
    want = eng.transcribe(E.AudioBuffer(cli.load_wav_file(wav), 16000))
    eng.close()
    for flag in ("auto", str(C)):
        r = subprocess.run([sys.executable, "-m", "openhush_amd.cli", "transcribe", wav, "--model-path", path, "--format", "json", "--audio-ctx", flag],
                           cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert json.loads(r.stdout)["text"] == want.text
    r = subprocess.run([sys.executable, "-m", "openhush_amd.cli", "transcribe", wav, "--model-path", path, "--audio-ctx", "64"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "window 0" in (r.stderr + r.stdout)
