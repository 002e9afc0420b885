"""Per-window audio context inside one batch (ohw_state_set_window_ctx) on the GPU.

Oracle comparisons follow tests/test_gpu_audio_ctx.py: the oracle is oracle.Model.synth with n_audio_ctx = n_ctx[b], fed the
GPU's own fetched log-mel with the frames from 2 * n_ctx[b] on zeroed (and, for the decoder, the GPU's own encoder rows);
the tolerances are that file's TOL_ACT and TOL_LOGIT, unchanged.  The stronger statement is bit-equality: the valid rows of
window b of a mixed batch are the rows of a fresh state that runs window b alone at ohw_state_set_audio_ctx(n_ctx[b]).
"""
import numpy as np
import pytest

from openhush_amd import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOL_ACT = {0: 6e-2, 1: 8e-3}
TOL_LOGIT = {0: 0.25, 1: 0.03}
MICRO = synth.PRESETS["micro"]
# envelope -> lengths: 8 is shorter than a query block, 63 has a masked key tail, 250 is no multiple of 8, one window sits at
# the envelope itself
MIXES = {256: [8, 63, 250, 256], 1500: [1500, 64, 750]}


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from openhush_amd import engine
    engine.lib()
    assert hasattr(engine.lib(), "ohw_state_set_window_ctx")
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

    def get(C):
        if C not in cache:
            hl = MICRO.as_list()
            hl[1] = C
            cache[C] = oracle.Model.synth(hl, 1234)
        return cache[C]
    yield get
    for m in cache.values():
        m.close()


def _pcm_batch():
    b = np.zeros(synth.CHUNK_SAMPLES, np.float32)
    b[:48000] = synth.synth_audio(3, 48000)
    return (np.stack([synth.synth_audio(7), b, synth.synth_audio(11), synth.synth_audio(13)]),
            [synth.CHUNK_SAMPLES, 48000, synth.CHUNK_SAMPLES, synth.CHUNK_SAMPLES])


PCM, NS = _pcm_batch()


def _cut(mel, C):
    z = mel.copy()
    z[:, 2 * C:] = 0
    return z


def _run_mix(E, st, env, lens, want=True):
    B = len(lens)
    st.set_audio_ctx(env)
    st.set_window_ctx(lens)
    mel = st.mel(PCM[:B], NS[:B], E.OHW_MEL_ZERO_TAIL, want=want)
    st.encode(B)
    return mel


def _mix(E, ctx, env, lens, max_batch=None):
    st = E.State(ctx, max_batch or len(lens))
    return st, _run_mix(E, st, env, lens)


def _prompt(ctx, B):
    return np.tile(np.asarray([ctx.tok.sot, ctx.tok.sot + 1, ctx.tok.transcribe], np.int32), (B, 1))


def _valid(st, what, lens):
    a = st.fetch(what, len(lens))
    return [a[b, :n].copy() for b, n in enumerate(lens)]


def _greedy(ctx, st, B, n_max=24):
    p = ctx.default_params()
    p.n_max = n_max
    return st.greedy_ex(B, p)


def _same_walk(x, y):
    return x["tokens"] == y["tokens"] and np.array_equal(x["logprobs"], y["logprobs"])


# ---------------------------------------------------------------------------------------------------------------------------
# 1. encoder against the oracle
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("env", [256, 1500])
def test_encoder_rows_match_each_windows_own_oracle(E, oracle, ctxs, omodel, dt, env):
    lens = MIXES[env]
    B = len(lens)
    st, mel = _mix(E, ctxs[dt], env, lens)
    assert st.audio_ctx == env and [st.window_ctx(b) for b in range(B)] == lens
    L = ctxs[dt].hp.n_text_layer
    got = {k: st.fetch(k, B) for k in ("stem", "block0", "enc", "xk0", f"xv{L - 1}")}
    assert got["enc"].shape == (B, env, MICRO.n_audio_state)          # the envelope's layout
    tol = TOL_ACT[dt]
    worst = {}
    for b, n in enumerate(lens):
        om = omodel(n)
        r_enc, _, r_stem, r_b0 = om.encode(_cut(mel[b], n), taps=True)
        s = oracle.State(om)
        s.set_encoder_output(got["enc"][b, :n])
        k, v = s.cross_kv()
        for name, ref, t in (("stem", r_stem, tol), ("block0", r_b0, 2 * tol), ("enc", r_enc, 2 * tol), ("xk0", k[0], 2 * tol),
                             (f"xv{L - 1}", v[L - 1], 2 * tol)):
            err = float(np.abs(got[name][b, :n] - ref).max())
            worst[name] = max(worst.get(name, 0.0), err)
            print(f"env {env} dtype {dt} window {b} n_ctx {n} {name}: max abs err {err:.5f} (tol {t})")
            assert err < t, (name, b, n, err, t)
    st.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. bit-equality with the uniform path, 3. no dependence on dead rows
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("env", [256, 1500])
def test_each_window_is_bit_equal_to_a_lone_uniform_run(E, ctxs, dt, env):
    ctx = ctxs[dt]
    lens = MIXES[env]
    B = len(lens)
    L = ctx.hp.n_text_layer
    st, _ = _mix(E, ctx, env, lens)
    whats = ("enc", "xk0", f"xv{L - 1}")
    rows = {w: _valid(st, w, lens) for w in whats}
    logits = st.decode(_prompt(ctx, B), [0] * B)
    walk = _greedy(ctx, st, B)
    for b, n in enumerate(lens):
        lone = E.State(ctx, 1)
        lone.set_audio_ctx(n)
        lone.set_batch_invariant(True)
        lone.mel(PCM[b:b + 1], NS[b:b + 1], E.OHW_MEL_ZERO_TAIL, want=False)
        lone.encode(1)
        for w in whats:
            a = lone.fetch(w, 1)[0]
            assert a.shape[0] == n and np.array_equal(a, rows[w][b]), (w, b, n)
        assert np.array_equal(lone.decode(_prompt(ctx, 1), [0])[0], logits[b]), (b, n)
        assert _same_walk(_greedy(ctx, lone, 1)[0], walk[b]), (b, n)
        lone.close()
    st.close()


@pytest.mark.parametrize("dt", [0, 1])
def test_valid_rows_do_not_depend_on_what_the_dead_rows_hold(E, ctxs, dt):
    ctx = ctxs[dt]
    env, lens = 256, MIXES[256]
    B = len(lens)
    L = ctx.hp.n_text_layer
    fresh, _ = _mix(E, ctx, env, lens)
    used = E.State(ctx, B)
    used.mel(PCM[::-1].copy(), NS[::-1], E.OHW_MEL_ZERO_TAIL, want=False)        # full-context audio in every buffer first
    used.encode(B)
    used.decode(_prompt(ctx, B), [0] * B)
    _run_mix(E, used, env, lens, want=False)
    for w in ("stem", "block0", "enc", "xk0", f"xv{L - 1}"):
        for b, (x, y) in enumerate(zip(_valid(fresh, w, lens), _valid(used, w, lens))):
            assert np.array_equal(x, y), (w, b)
    assert np.array_equal(fresh.decode(_prompt(ctx, B), [0] * B), used.decode(_prompt(ctx, B), [0] * B))
    for x, y in zip(_greedy(ctx, fresh, B), _greedy(ctx, used, B)):
        assert _same_walk(x, y)
    fresh.close()
    used.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. every cross-attention form under lengths
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [1, 0])
def test_every_cross_attention_form_runs_under_lengths(E, oracle, ctxs, omodel, dt):
    ctx = ctxs[dt]
    env, lens = 256, [8, 250, 256]
    st, _ = _mix(E, ctx, env, lens, 15)
    st.set_persistent(True)                        # never used while lengths are set
    enc = _valid(st, "enc", lens)

    def ostate(b):                                 # a fresh oracle decoder of window b's own context on the GPU's encoder rows
        s = oracle.State(omodel(lens[b]))
        s.set_encoder_output(enc[b])
        return s
    rng = np.random.default_rng(5)
    forced = [ctx.tok.sot, ctx.tok.sot + 1, ctx.tok.transcribe, ctx.tok.timestamp_begin] + [int(t) for t in rng.integers(1000, 30000, 4)]
    ref_all = [ostate(b).decode(forced, 0, all_pos=True) for b in range(3)]
    tol = TOL_LOGIT[dt]
    worst = 0.0
    for n_new in (1, 2, 3, 4):                     # plain, rows2, rows3, rows4: positions 0 .. n_new - 1, then one more token
        lg = st.decode(np.tile(np.asarray(forced[:n_new], np.int32), (3, 1)), [0, 0, 0])
        lg1 = st.decode(np.full((3, 1), forced[n_new], np.int32), [n_new] * 3)
        for b in range(3):
            worst = max(worst, float(np.abs(lg[b] - ref_all[b][n_new - 1]).max()), float(np.abs(lg1[b] - ref_all[b][n_new]).max()))
    print(f"\nlengths {lens} dtype {dt}: worst teacher-forced logit err {worst:.4f} (tol {tol})")
    assert worst < tol, worst
    # decode_active: the inactive window is skipped, the others keep their bits
    full = st.decode(np.full((3, 1), 1234, np.int32), [5, 5, 5])
    part = st.decode_active(np.full((3, 1), 1234, np.int32), [5, 5, 5], [1, 0, 1])
    assert np.array_equal(part[0], full[0]) and np.array_equal(part[2], full[2]) and not part[1].any()
    # beam search, K = 2..5: the oracle's sequence, or one that scores within the rule of tests/test_gpu_audio_ctx.py
    bias = np.zeros(MICRO.n_vocab, np.float32)
    om0 = omodel(lens[0])
    bias[om0.tok_beg:] = 6.0
    bias[om0.tok_eot] = 27.0
    st.set_logit_bias(bias)
    p = ctx.default_params()
    p.n_max = 12
    for K in (2, 3, 4, 5):
        got = st.beam_search(3, K, p)
        assert st.beam_search(3, K, p) == got
        for w, n in enumerate(lens):
            om = omodel(n)
            op = om.default_params()
            op.n_max = 12
            ref = oracle.beam_search(om, enc[w], op, K, bias)
            g = got[w]
            assert len(g["tokens"]) > 0
            if g["tokens"] != ref["tokens"]:
                best = max(c[1] / max(1, len(c[0])) for c in ref["candidates"])
                mine = max(ostate(w).score_sequence(op, g["tokens"], e, bias) / max(1, len(g["tokens"])) for e in (True, False))
                assert mine > best - (0.1 if dt == 0 else 0.02), (K, w, g, ref["tokens"], mine, best)
    st.set_logit_bias(None)
    # one rung of the temperature ladder on the device with window 1 inactive: every draw has the oracle's log-probability
    cap = ctx.hp.n_text_ctx
    u = np.random.default_rng(3).random((3, cap))
    p2 = ctx.default_params()
    p2.n_max = 16
    res = st.sample_pass(3, 0.4, [1, 0, 1], u, p2)
    assert res[1]["tokens"] == [] and len(res[0]["tokens"]) > 0 and len(res[2]["tokens"]) > 0
    for b in (0, 2):
        om = omodel(lens[b])
        op2 = om.default_params()
        op2.n_max = 16
        frc = res[b]["tokens"] + ([om.tok_eot] if res[b]["ended_by_eot"] else [])
        r = ostate(b).decode_pass(op2, None, 0.4, oracle.MT19937(0), frc)
        for i in range(len(res[b]["tokens"])):
            assert abs(float(r["plogs"][i]) - float(res[b]["logprobs"][i])) < 2 * TOL_LOGIT[dt] / 0.4, (b, i)
    # language detection: one decoder step under the lengths
    ids, probs = st.detect_language(3)
    for b, n in enumerate(lens):
        om = omodel(n)
        lg = ostate(b).decode([om.tok_sot], 0)
        lang = lg[om.tok_sot + 1: om.tok_sot + 1 + probs.shape[1]]
        top2 = np.sort(lang)[-2:]
        assert int(ids[b]) == int(lang.argmax()) or top2[1] - top2[0] < 2 * TOL_LOGIT[dt]
        assert abs(float(probs[b].sum()) - 1.0) < 1e-3
    for name in ("plain", "rows2", "rows3", "rows4", "group2", "group3", "group4", "group5"):
        assert st.counter("xattn." + name) > 0, name
    assert st.counter("xattn.split") == 0 and st.counter("xattn.group_split") == 0 and st.counter("persist_launches") == 0
    st.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. graph reuse, 6. refusals, 7. slices
# ---------------------------------------------------------------------------------------------------------------------------
def test_one_step_graph_serves_every_mix_of_an_envelope(E, ctxs):
    ctx = ctxs[1]
    uni = E.State(ctx, 3)
    uni.set_audio_ctx(256)
    uni.mel(PCM[:3], NS[:3], E.OHW_MEL_ZERO_TAIL, want=False)
    uni.encode(3)
    uniform = _greedy(ctx, uni, 3)
    uni.set_batch_invariant(True)                                # the variant choice lengths imply
    uniform_inv = _greedy(ctx, uni, 3)
    st = E.State(ctx, 3)
    _run_mix(E, st, 256, [8, 250, 256], want=False)
    c0 = st.counter("step_captures")
    a = _greedy(ctx, st, 3)
    c1 = st.counter("step_captures")
    assert c1 == c0 + 1
    _run_mix(E, st, 256, [256, 63, 8], want=False)
    b = _greedy(ctx, st, 3)
    assert st.counter("step_captures") == c1                     # the lengths are read from device memory, not captured
    assert _same_walk(a[2], uniform_inv[2]) and _same_walk(b[0], uniform_inv[0])      # the windows that sit at the envelope
    assert not _same_walk(a[0], b[0])
    _run_mix(E, st, 256, [8, 250, 256], want=False)
    assert all(_same_walk(x, y) for x, y in zip(_greedy(ctx, st, 3), a)) and st.counter("step_captures") == c1
    st.set_window_ctx(None)                                      # back to the uniform graph and the uniform bits
    st.mel(PCM[:3], NS[:3], E.OHW_MEL_ZERO_TAIL, want=False)
    st.encode(3)
    assert [st.window_ctx(i) for i in range(3)] == [256] * 3
    back = _greedy(ctx, st, 3)
    c2 = st.counter("step_captures")
    assert c2 == c1 + 1
    assert all(_same_walk(x, y) for x, y in zip(back, uniform))
    _run_mix(E, st, 256, [8, 250, 256], want=False)
    _greedy(ctx, st, 3)
    assert st.counter("step_captures") == c2
    uni.close()
    st.close()


def test_bad_lengths_and_stale_stages_are_refused(E, ctxs):
    ctx = ctxs[1]
    L = E.lib()
    st = E.State(ctx, 3)
    st.set_audio_ctx(256)
    arr = lambda v: np.asarray(v, np.int32)      # noqa: E731
    for bad in ([8, 0, 256], [8, 257, 256], [-1]):
        a = arr(bad)
        assert L.ohw_state_set_window_ctx(st.h, E._ip(a), a.size) == E.OHW_E_INVALID_ARG, bad
    a = arr([8, 8, 8, 8])
    assert L.ohw_state_set_window_ctx(st.h, E._ip(a), 4) == E.OHW_E_INVALID_ARG          # above max_batch
    _run_mix(E, st, 256, [8, 250, 256], want=False)
    good = st.decode(_prompt(ctx, 3), [0, 0, 0])
    p = ctx.default_params()
    p.n_max = 4
    one = np.full((3, 1), ctx.tok.sot, np.int32)
    decodes = (lambda: st.decode(one, [0, 0, 0]), lambda: st.decode_active(one, [0, 0, 0], [1, 1, 1]), lambda: st.greedy(3, p),
               lambda: st.greedy_ex(3, p), lambda: st.detect_language(3),
               lambda: st.sample_pass(3, 0.5, [1, 1, 1], np.zeros((3, ctx.hp.n_text_ctx)), p))

    def refused(f):
        with pytest.raises(E.WhisperError) as ex:
            f()
        assert ex.value.code == E.OHW_E_INVALID_ARG

    st.set_window_ctx([8, 250, 255])             # the lengths changed, no encode since: no decode entry may read the K/V
    for f in decodes:
        refused(f)
    refused(lambda: st.encode(3))                # ... and no encode may read the mel image of other lengths
    st.set_window_ctx(None)
    for f in decodes:
        refused(f)
    refused(lambda: st.encode(3))
    st.set_window_ctx([8, 250, 256])             # the lengths of the last mel and encode again: fine
    assert np.array_equal(st.decode(_prompt(ctx, 3), [0, 0, 0]), good)
    st.set_window_ctx([8, 250])                  # lengths for two windows, a mel of three
    refused(lambda: st.mel(PCM[:3], NS[:3], E.OHW_MEL_ZERO_TAIL, want=False))
    st.set_window_ctx([8, 250, 256])
    st.set_audio_ctx(128)                        # a new envelope clears the lengths
    st.set_audio_ctx(256)
    refused(lambda: st.decode(one, [0, 0, 0]))
    st.close()


def test_slices_record_their_lengths_into_their_slots(E, ctxs):
    ctx = ctxs[0]
    env, lens = 256, [63, 250, 8]
    L = ctx.hp.n_text_layer
    one, _ = _mix(E, ctx, env, lens)
    two = E.State(ctx, 3)
    two.set_audio_ctx(env)
    two.set_window_ctx(lens[:2])
    two.mel(PCM[:2], NS[:2], E.OHW_MEL_ZERO_TAIL, want=False)
    two.encode_slice(2, 0, 3)
    two.set_window_ctx(lens[2:])
    two.mel(PCM[2:3], NS[2:3], E.OHW_MEL_ZERO_TAIL, want=False)
    two.encode_slice(1, 2, 3)
    assert [two.window_ctx(b) for b in range(3)] == lens
    for what in ("xk0", f"xv{L - 1}"):
        for b, (x, y) in enumerate(zip(_valid(one, what, lens), _valid(two, what, lens))):
            assert np.array_equal(x, y), (what, b)
    assert np.array_equal(one.decode(_prompt(ctx, 3), [0, 0, 0]), two.decode(_prompt(ctx, 3), [0, 0, 0]))
    # a later slice without lengths beside slices with lengths is refused
    two.set_window_ctx(None)
    two.mel(PCM[2:3], NS[2:3], E.OHW_MEL_ZERO_TAIL, want=False)
    with pytest.raises(E.WhisperError) as ex:
        two.encode_slice(1, 2, 3)
    assert ex.value.code == E.OHW_E_INVALID_ARG
    one.close()
    two.close()
