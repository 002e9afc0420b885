"""Prompted decoding on the GPU: ohw_state_set_window_prompt / ohw_state_prefill and the decode entries under a context table.

The oracle is fed the GPU's own encoder output and the WHOLE sequence ([prev], the context, the sot prompt, the forced tokens) at
position 0; the GPU reads the context through the prefill (chunks of 8 positions, no logits) and then decodes from
n_past = len[b].  Tolerance: TOL_LOGIT and the pick rule of tests/test_gpu_decoder_depth.py.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from openhush_amd import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOL_LOGIT = {0: 0.25, 1: 0.03}           # tests/test_gpu_decoder_depth.py
CTX_LENS = [0, 1, 7, 8, 223]             # tokens per window: 8 tokens occupy exactly 9 positions, 223 is the cap (n_text_ctx / 2 - 1)
N_FORCED = 6
HERE = os.path.dirname(os.path.abspath(__file__))


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


def _check_row(got, ref, tol, where):
    err = float(np.abs(got - ref).max())
    assert err < tol, (where, err)
    if int(got.argmax()) != int(ref.argmax()):
        top = np.sort(ref)[-2:]
        assert top[1] - top[0] < 2 * tol, (where, int(got.argmax()), int(ref.argmax()), float(top[1] - top[0]))
    return err


def _contexts(tok, lens, seed=11):
    rng = np.random.default_rng(seed)
    return [[int(t) for t in rng.integers(0, tok.eot, size=n)] for n in lens]


def _forced(tok, seed, n=N_FORCED):
    rng = np.random.default_rng(seed)
    return [int(t) for t in rng.integers(0, tok.eot, size=n)]


def _pcm(B):
    return np.stack([synth.synth_audio(i) for i in range(B)])


def _state(E, preset, dt, B, mode, pcm=None):
    hp = synth.PRESETS[preset]
    ctx = E.Context.synthetic(hp.as_list(), 1234, 0, dt)
    st = E.State(ctx, B)
    if mode == "invariant":
        st.set_batch_invariant(True)
    if mode == "var":
        st.set_window_ctx([hp.n_audio_ctx] * B)      # full lengths: the per-window kernels, the uniform model for the oracle
    st.mel(_pcm(B) if pcm is None else pcm, None, E.OHW_MEL_ZERO_TAIL, want=False)
    st.encode(B)
    return ctx, st


def logits_case(E, oracle, preset, dt, mode, xa_on=True):
    """prefill + teacher-forced decode of 5 windows against the oracle; returns the worst error"""
    B = len(CTX_LENS)
    ctx, st = _state(E, preset, dt, B, mode)
    om = oracle.Model.synth(synth.PRESETS[preset].as_list(), 1234)
    tok = ctx.tok
    ctxs = _contexts(tok, CTX_LENS)
    prompt = [tok.sot, tok.sot + 1, tok.transcribe, tok.timestamp_begin]
    enc = st.fetch("enc", B)
    st.set_window_prompt(ctxs)
    lens = [st.window_prompt_len(b) for b in range(B)]
    assert lens == [0 if n == 0 else n + 1 for n in CTX_LENS]
    seqs, refs = [], []
    for b in range(B):
        seq = ([tok.prev] + ctxs[b] if ctxs[b] else []) + prompt + _forced(tok, 100 + b)
        s = oracle.State(om)
        s.set_encoder_output(enc[b])
        refs.append(s.decode(seq, 0, all_pos=True))
        seqs.append(seq)
    before = st.counter("xattn.chunk")
    st.prefill(B)
    chunks = st.counter("xattn.chunk") - before
    want_chunk = xa_on and mode in ("invariant", "var")          # 5 windows x 4 heads < 256: the chunk kernel needs one of the two
    assert chunks == (28 * synth.PRESETS[preset].n_text_layer if want_chunk else 0), (mode, xa_on, chunks)
    tol, worst = TOL_LOGIT[dt], 0.0
    lg = st.decode(np.asarray([s[n:n + 4] for s, n in zip(seqs, lens)], np.int32), lens)
    for b in range(B):
        worst = max(worst, _check_row(lg[b], refs[b][lens[b] + 3], tol, (mode, b, "prompt")))
    for i in range(N_FORCED):
        pos = [n + 4 + i for n in lens]
        lg = st.decode(np.asarray([[s[p]] for s, p in zip(seqs, pos)], np.int32), pos)
        for b in range(B):
            worst = max(worst, _check_row(lg[b], refs[b][pos[b]], tol, (mode, b, i)))
    print(f"prompt logits {preset} dtype {dt} {mode} xa={int(xa_on)}: worst error {worst:.4f} (tol {tol})")
    om.close()
    return worst


@pytest.mark.parametrize("mode", ["plain", "invariant", "var"])
@pytest.mark.parametrize("preset,dt", [("micro", 0), ("micro", 1), ("micro-v3", 1)])
def test_logits_behind_a_context_match_the_oracle(E, oracle, preset, dt, mode):
    logits_case(E, oracle, preset, dt, mode)


@pytest.mark.parametrize("xa", ["0", "1"])
def test_logits_with_the_prefill_knob_in_a_child_process(xa):
    """OHW_PREFILL_XA is read when a state is created: 0 sends the chunks through the existing kernels, 1 (the default) through
    cross_attn_chunk_kernel; both match the oracle"""
    env = dict(os.environ, OHW_PREFILL_XA=xa)
    code = f"import sys; sys.path[:0] = [{os.path.dirname(HERE)!r}, {HERE!r}]; import test_gpu_prompt as t; t.child({xa!r})"
    r = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(HERE), env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "child ok" in r.stdout


def test_a_window_does_not_depend_on_its_batch(E):
    """batch-invariant mode: the window with 7 context tokens gives the same bits alone and in the batch of 5; the window without
    context gives the bits of a state with no table"""
    B, dt = len(CTX_LENS), 1
    ctx, st = _state(E, "micro", dt, B, "invariant")
    tok = ctx.tok
    ctxs = _contexts(tok, CTX_LENS)
    prompt = [tok.sot, tok.sot + 1, tok.transcribe, tok.timestamp_begin]
    st.set_window_prompt(ctxs)
    st.prefill(B)
    lens = [st.window_prompt_len(b) for b in range(B)]
    full = st.decode(np.asarray([prompt] * B, np.int32), lens).copy()
    nxt = st.decode(np.asarray([[7]] * B, np.int32), [n + 4 for n in lens]).copy()
    pcm = _pcm(B)
    _, one = _state(E, "micro", dt, 1, "invariant", pcm=pcm[2:3])
    one.set_window_prompt([ctxs[2]])
    one.prefill(1)
    assert np.array_equal(one.decode(np.asarray([prompt], np.int32), [lens[2]])[0], full[2])
    assert np.array_equal(one.decode(np.asarray([[7]], np.int32), [lens[2] + 4])[0], nxt[2])
    _, bare = _state(E, "micro", dt, 1, "invariant", pcm=pcm[0:1])
    bare.prefill(1)                                   # no table: a no-op
    assert np.array_equal(bare.decode(np.asarray([prompt], np.int32), [0])[0], full[0])
    assert np.array_equal(bare.decode(np.asarray([[7]], np.int32), [4])[0], nxt[0])


def test_greedy_behind_a_context(E, oracle):
    """greedy_ex under a table: the context is not in the returned tokens, every pick is the oracle's (walked with the context in
    front) or within twice the logit tolerance of it, window 0 (no context) equals a run without a table, and other lengths
    capture no new graph"""
    B, dt = 3, 1
    ctx, st = _state(E, "micro", dt, B, "invariant")
    om = oracle.Model.synth(synth.PRESETS["micro"].as_list(), 1234)
    tok = ctx.tok
    p = ctx.default_params()
    p.n_max = 10
    plain = st.greedy_ex(B, p)
    caps = st.counter("step_captures")
    ctxs = _contexts(tok, [0, 5, 40], seed=5)
    st.set_window_prompt(ctxs)
    got = st.greedy_ex(B, p)
    assert st.counter("step_captures") == caps
    st.set_window_prompt(_contexts(tok, [3, 0, 17], seed=6))
    st.greedy_ex(B, p)
    assert st.counter("step_captures") == caps                    # positions are device data
    st.set_window_prompt(ctxs)
    again = st.greedy_ex(B, p)
    assert [g["tokens"] for g in again] == [g["tokens"] for g in got]
    assert got[0]["tokens"] == plain[0]["tokens"] and np.array_equal(got[0]["logprobs"], plain[0]["logprobs"])
    enc = st.fetch("enc", B)
    op = om.default_params()
    op.n_max = 10
    prompt = om.build_prompt(op)
    tol = TOL_LOGIT[dt]
    for b in range(B):
        toks = got[b]["tokens"]
        assert 1 <= len(toks) <= 10
        head = ([tok.prev] + ctxs[b]) if ctxs[b] else []
        s = oracle.State(om)
        s.set_encoder_output(enc[b])
        lg = s.decode(head + prompt + toks, 0, all_pos=True)
        for i, t in enumerate(toks):
            pick, _, filt, _ = om.process_logits(op, lg[len(head) + len(prompt) - 1 + i], toks[:i])
            assert pick == t or filt[pick] - filt[t] < 2 * tol, (b, i, pick, t, float(filt[pick] - filt[t]))
    st.set_window_prompt(None)
    assert [g["tokens"] for g in st.greedy_ex(B, p)] == [g["tokens"] for g in plain]
    om.close()


def test_beam_search_behind_a_context(E, oracle):
    """beam 5, contexts [0, 40]: the window without context equals a run with no table bit for bit (batch-invariant mode); the
    other's best sequence, scored by an oracle walk behind the context, has the sum the GPU reports: every token's log-probability
    agrees within the bound of tests/test_gpu_beam.py, (0.5 | 0.06) * sqrt(tokens)"""
    W, K, dt = 2, 5, 1
    hp = synth.PRESETS["micro"]
    ctx = E.Context.synthetic(hp.as_list(), 1234, 0, dt)
    st = E.State(ctx, W * K)
    st.set_batch_invariant(True)
    st.mel(_pcm(W), None, E.OHW_MEL_ZERO_TAIL, want=False)
    st.encode(W)
    om = oracle.Model.synth(hp.as_list(), 1234)
    p = ctx.default_params()
    p.n_max = 8
    plain = st.beam_search(W, K, p)
    ctxs = _contexts(ctx.tok, [0, 40], seed=9)
    st.set_window_prompt(ctxs)
    got = st.beam_search(W, K, p)
    assert got[0]["tokens"] == plain[0]["tokens"] and got[0]["sum_logprob"] == plain[0]["sum_logprob"]
    op = om.default_params()
    op.n_max = 8
    prompt = om.build_prompt(op)
    toks = got[1]["tokens"]
    assert 1 <= len(toks) <= 8
    head = [ctx.tok.prev] + ctxs[1]
    s = oracle.State(om)
    s.set_encoder_output(st.fetch("enc", W)[1])
    lg = s.decode(head + prompt + toks, 0, all_pos=True)
    sums = [0.0]
    for i, t in enumerate(toks + [ctx.tok.eot]):
        row = lg[len(head) + len(prompt) - 1 + i] if i < len(toks) else s.decode(head + prompt + toks, 0)
        _, _, _, lps = om.process_logits(op, row, toks[:i])
        sums.append(sums[-1] + float(lps[t]))
    # which sum ohw_beam_search reports: a sequence shorter than n_max left the loop through end-of-text (the finished pool: its
    # sum includes that token's log-probability); one of n_max tokens was still live (no end-of-text in its sum)
    want = sums[-1] if len(toks) < 8 else sums[-2]
    err = abs(got[1]["sum_logprob"] - want)
    bound = (0.5 if dt == 0 else 0.06) * max(1, len(toks)) ** 0.5            # tests/test_gpu_beam.py's bound
    print(f"beam behind a context: {len(toks)} tokens, GPU sum {got[1]['sum_logprob']:.4f}, oracle {want:.4f}: error {err:.5f} (bound {bound:.4f})")
    assert err < bound
    om.close()


def test_beam_search_windows_with_unequal_contexts_do_not_touch_each_other(E):
    """cache row w (1 <= w < W) holds window w's context after the prefill AND is the own row of a beam of window w / K, which
    writes from its own (shorter) past's end upward: the search must keep window w's shared past where only w's beams write.
    Batch-invariant mode: a window behind 40 tokens gives the same bits whatever its neighbours' contexts are - against the
    batch where all contexts have that length (there a neighbour's beams write behind the shared pasts, as without a table)"""
    W, K, dt = 3, 5, 1
    hp = synth.PRESETS["micro"]
    ctx = E.Context.synthetic(hp.as_list(), 1234, 0, dt)
    st = E.State(ctx, W * K)
    st.set_batch_invariant(True)
    st.mel(_pcm(W), None, E.OHW_MEL_ZERO_TAIL, want=False)
    st.encode(W)
    p = ctx.default_params()
    p.n_max = 12
    c = _contexts(ctx.tok, [40, 40, 40], seed=9)
    st.set_window_prompt(c)
    same = st.beam_search(W, K, p)
    for lens in ([0, 40, 40], [0, 3, 40], [40, 0, 40], [7, 40, 0], [40, 40, 0]):
        st.set_window_prompt([c[w][:n] for w, n in enumerate(lens)])
        got = st.beam_search(W, K, p)
        for w, n in enumerate(lens):
            if n == 40:
                assert got[w]["tokens"] == same[w]["tokens"] and got[w]["sum_logprob"] == same[w]["sum_logprob"], (lens, w, got[w], same[w])
    st.set_window_prompt(None)
    plain = st.beam_search(W, K, p)
    st.set_window_prompt([[], c[1], []])
    got = st.beam_search(W, K, p)
    assert [g["tokens"] for g in (got[0], got[2])] == [g["tokens"] for g in (plain[0], plain[2])]


KERNEL_EDGE_GAP = 1e-5        # tests/test_gpu_device_ladder.py: a different pick only where the draw is this close to an interval edge


def _host_probs(E, ctx, p, row, hist, T):
    """tests/test_gpu_device_ladder.py: what ohw_sample_host hands std::discrete_distribution"""
    import ctypes as C
    f = (row.astype(np.float32) / np.float32(T)).astype(np.float32)
    c = np.asarray(hist or [0], np.int32)
    lp = C.c_float(0)
    tok = E.lib().ohw_sample_greedy_host(ctx.h, C.byref(p), E._fp(f), E._ip(c), len(hist), C.byref(lp))
    lse = np.float32(f[tok] - np.float32(lp.value))
    return np.where(f == -np.inf, np.float32(0), np.exp((f - lse).astype(np.float32))).astype(np.float32)


def _edge_gap(probs, u):
    pd = probs.astype(np.float64)
    cp = np.cumsum(pd / pd.sum())
    cp[-1] = 1.0
    k = int(np.searchsorted(cp, u, side="left"))
    return float(min(u - (cp[k - 1] if k > 0 else 0.0), cp[k] - u))


def test_sample_pass_behind_a_context_equals_the_host_ladder(E):
    """a temperature pass on the device (pre-drawn uniforms) with a table against the host-sampled ladder's path: prefill for the
    active windows, the prompt at past = len[b], ohw_sample_host draw by draw from the same generators.  The same tokens, except
    from a step on whose draw lies within KERNEL_EDGE_GAP of an interval edge of the host's distribution.  Window 1 is inactive"""
    B, dt, T = 4, 1, 0.4
    ctx, st = _state(E, "micro", dt, B, "plain")
    tok = ctx.tok
    p = ctx.default_params()
    p.n_max = 8
    ctxs = _contexts(tok, [0, 9, 7, 30], seed=21)
    active = [1, 0, 1, 1]
    st.set_window_prompt(ctxs)
    lens = [st.window_prompt_len(b) for b in range(B)]
    cap = ctx.hp.n_text_ctx
    u = np.stack([E.HostRng(50 + b).uniforms(cap) for b in range(B)])
    dev = st.sample_pass(B, T, active, u, p)
    assert dev[1]["tokens"] == []
    prompt = [tok.sot, tok.sot + 1, tok.transcribe]
    st.prefill(B, active)
    gens = [E.HostRng(50 + b) for b in range(B)]
    hist = [[] for _ in range(B)]
    live = list(active)
    excused = [False] * B
    lg = st.decode_active(np.asarray([prompt] * B, np.int32), lens, active)
    npast = [n + len(prompt) for n in lens]
    for i in range(p.n_max):
        feed = [tok.eot] * B
        for b in range(B):
            if not live[b]:
                continue
            probs = _host_probs(E, ctx, p, lg[b], hist[b], T)
            t, _, _ = ctx.sample_host(p, lg[b].copy(), hist[b], T, gens[b])
            if not excused[b] and i < len(dev[b]["tokens"]) + (1 if dev[b]["ended_by_eot"] else 0):
                d = dev[b]["tokens"][i] if i < len(dev[b]["tokens"]) else tok.eot
                if d != t:
                    assert _edge_gap(probs, u[b][i]) < KERNEL_EDGE_GAP, (b, i, d, t)
                    excused[b] = True
            if t == tok.eot or len(hist[b]) + 1 >= p.n_max:
                if t != tok.eot:
                    hist[b].append(t)
                live[b] = 0
            else:
                hist[b].append(t)
                feed[b] = t
        if not any(live):
            break
        lg = st.decode_active(np.asarray([[t] for t in feed], np.int32), npast, live)
        npast = [n + (1 if live[b] else 0) for b, n in enumerate(npast)]
    for b in range(B):
        if active[b] and not excused[b]:
            assert dev[b]["tokens"] == hist[b], (b, dev[b]["tokens"], hist[b])
    print("sample_pass behind a context:", [d["tokens"] for d in dev], "excused", excused)


def engine_child(model_path):
    """the body of test_engine_layers_in_a_child_process.  Under whisper.cpp's default policy the synthetic model's windows fail the
    acceptance test at every temperature and end at T = 1.0, where the rule has dropped the prompt: last_tokens is then the same
    with and without a prompt.  So under the default policy the T = 0 pass is compared through last_trace, and the last_tokens
    checks the issue names run with temperature_inc = 0 (every window kept at T = 0)"""
    import json
    import tempfile
    import wave
    from openhush_amd import engine as E, streaming as S
    pcms = [synth.synth_audio(60 + i)[:16000 * (8 + 3 * i)] for i in range(3)]
    eng = E.WhisperEngine.new(model_path, "en", False, True, 0, E.OHW_DTYPE_F16, 4)

    def run(a):
        eng.transcribe(E.AudioBuffer(a.copy(), 16000))
        return eng.last_tokens()
    # the whole ladder first (whisper.cpp's default policy): the passes with T < 0.5 decode behind the prompt, so the T = 0 pass
    # changes; a window that falls through to T >= 0.5 decodes without it from there on
    run(pcms[0])
    trace_plain = eng.last_trace()
    eng.set_initial_prompt([5, 6, 7, 8, 9, 10, 11] * 4)
    run(pcms[0])
    trace_prompted = eng.last_trace()
    assert trace_plain[0][1] == 0.0 and trace_prompted[0][1] == 0.0
    assert trace_prompted[0][2] != trace_plain[0][2], "the prompt does not reach the T = 0 pass"
    print("passes without / with a prompt:", [t for _, t, _ in trace_plain], [t for _, t, _ in trace_prompted])
    eng.set_initial_prompt(None)
    # every window kept at T = 0: last_tokens is what was decoded behind the prompt
    eng.set_decode_policy(temperature_inc=0.0)
    plain = run(pcms[0])
    eng.set_initial_prompt(" w1 w2, OpenHush 42")                 # text: tokenized on the host
    texted = run(pcms[0])
    eng.set_initial_prompt([5, 6, 7, 8, 9, 10, 11] * 40)          # 280 tokens: clipped to the last n_text_ctx / 2 - 1
    prompted = run(pcms[0])
    assert prompted != plain, "the prompt does not reach the decoder"
    assert texted != plain
    # transcribe_batch of three recordings behind the prompt equals each submitted alone
    alone = [run(a) for a in pcms]
    res = eng.transcribe_batch([E.AudioBuffer(a.copy(), 16000) for a in pcms])
    assert [eng.batch_result(i)[1] for i in range(3)] == alone, "transcribe_batch differs from each alone"
    assert len(res) == 3
    eng.set_initial_prompt("")
    assert run(pcms[0]) == plain, "clearing the prompt does not restore the unprompted tokens"
    eng.close()
    # StreamingSession(carry_context=True): chunk 1's text tokens are chunk 2's context
    ctx = E.Context.from_file(model_path, 0, E.OHW_DTYPE_F16)
    p = ctx.default_params()
    p.n_max = 10
    rec = np.concatenate([synth.synth_audio(71)[:16000 * 5], synth.synth_audio(72)[:16000 * 5]])
    ses = S.StreamingSession(ctx, beam_size=0, params=p, carry_context=True)
    ses.tick(rec, 16000 * 5)
    first = list(ses.context)
    assert ses.state.window_prompt_len(0) == 0 and len(first) > 0           # chunk 1 had no context
    ses.tick(rec, len(rec), is_final=True)
    assert ses.state.window_prompt_len(0) == len(first) + 1                 # chunk 2 decoded behind [prev] + chunk 1's tokens
    off = S.StreamingSession(ctx, beam_size=0, params=p)
    off.tick(rec, 16000 * 5)
    off.tick(rec, len(rec), is_final=True)
    assert off.state.window_prompt_len(0) == 0 and off.context == []
    # the CLI's --prompt reaches the engine: other tokens, so another text, than without it
    with tempfile.TemporaryDirectory() as d:
        wav = os.path.join(d, "a.wav")
        with wave.open(wav, "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
            w.writeframes((np.clip(pcms[0], -1, 1) * 32767).astype("<i2").tobytes())
        from openhush_amd import cli

        def cli_text(extra):
            r = subprocess.run([sys.executable, "-m", "openhush_amd.cli", "transcribe", wav, "--model-path", model_path, "--language", "en", "--dtype", "f16",
                                "--format", "json"] + extra, cwd=os.path.dirname(HERE), capture_output=True, text=True, timeout=240)
            assert r.returncode == 0, r.stderr[-2000:]
            return json.loads(r.stdout)["text"]
        eng2 = E.WhisperEngine.new(model_path, "en", False, True, 0, E.OHW_DTYPE_F16, 8)
        a = E.AudioBuffer(cli.load_wav_file(wav), 16000)
        want_plain = eng2.transcribe(a).text
        trace0 = eng2.last_trace()
        eng2.set_initial_prompt("w5 w6 w7, 1 2 3")
        want_prompted = eng2.transcribe(E.AudioBuffer(cli.load_wav_file(wav), 16000)).text
        assert cli_text([]) == want_plain
        assert eng2.last_trace()[0][2] != trace0[0][2]              # the prompt changed the T = 0 pass of the engine the CLI mirrors
        assert cli_text(["--prompt", "w5 w6 w7, 1 2 3"]) == want_prompted
    print("child ok")


def test_engine_layers_in_a_child_process(tmp_models):
    """small preset: set_initial_prompt (text and tokens) changes last_tokens and "" restores them bit for bit, transcribe_batch
    of three equals each alone, StreamingSession(carry_context=True) feeds chunk 1's tokens as chunk 2's context, the CLI's
    --prompt reaches the engine"""
    path = tmp_models("small")
    code = f"import sys; sys.path[:0] = [{os.path.dirname(HERE)!r}, {HERE!r}]; import test_gpu_prompt as t; t.engine_child({path!r})"
    r = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(HERE), capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "child ok" in r.stdout


def test_refusals(E):
    ctx, st = _state(E, "micro", 1, 2, "plain")
    cap = ctx.hp.n_text_ctx // 2 - 1

    def refused(word, fn):
        with pytest.raises(E.WhisperError) as ei:
            fn()
        assert ei.value.code == E.OHW_E_INVALID_ARG and word in str(ei.value), str(ei.value)
    refused("is outside", lambda: st.set_window_prompt([[1, ctx.hp.n_vocab], []]))
    refused("is outside", lambda: st.set_window_prompt([[-1], []]))
    refused("context tokens", lambda: st.set_window_prompt([[1] * (cap + 1), []]))
    refused("max_batch", lambda: st.set_window_prompt([[1], [], [2]]))
    assert st.window_prompt_len(0) == 0                      # nothing was set
    st.set_window_prompt([[1] * cap, []])
    assert [st.window_prompt_len(b) for b in range(2)] == [cap + 1, 0]
    refused("batch of the last", lambda: st.prefill(1))
    st.set_window_prompt([[1, 2]])                           # a table for one window, a decode batch of two
    refused("named 1 windows", lambda: st.prefill(2))
    refused("named 1 windows", lambda: st.greedy_ex(2))
    st.set_window_prompt(None)
    st.prefill(1)                                            # no table: a no-op, whatever the batch


def child(xa):
    """the body of test_logits_with_the_prefill_knob_in_a_child_process: OHW_PREFILL_XA is in the environment"""
    from openhush_amd import engine as _E
    from oracle import oracle as _o
    _o.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    for mode in ("invariant", "var"):
        logits_case(_E, _o, "micro", 1, mode, xa_on=xa != "0")
    logits_case(_E, _o, "micro", 0, "var", xa_on=xa != "0")
    print("child ok")
