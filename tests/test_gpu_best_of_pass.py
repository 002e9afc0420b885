"""ohw_sample_pass_n: one temperature pass with N candidates per window on the resident cross K/V (best-of sampling), micro
model, W <= 3 windows, N in {2, 3, 5}, max_batch = W * N.

The candidates of a window share the prefill's and the prompt's self K/V through a slot table and the window's cross K/V; what
can go wrong is a candidate reading another row's cache, another window's K/V, or a flag of the wrong granularity.  So: equal
draws must give equal rows, permuted draws permuted rows, a window in a batch of unequal contexts the rows it gives alone (word
for word, under the batch-invariant kernel choice), inactive windows nothing, and the entries that follow the bits they gave
before.  Every candidate is then walked teacher-forced on the oracle under test_gpu_policy._walk_and_compare's per-step rule
(that function itself replays an engine trace from one generator per window; a candidate j draws from generator j, so the walk
is restated here with its thresholds imported unchanged).  Bit equality with ohw_sample_pass is not asserted: the group path
runs cross_attn_rows_kernel, the single path cross_attn_kernel."""
import numpy as np
import pytest

from openhush_amd import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

T_PASS = 0.6
N_MAX = 24


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


SEEDS = (7, 3, 11)


def _pcm(ws):
    return np.stack([synth.synth_audio(SEEDS[w]) for w in ws])


def _bias(ctx, ts_b=6.0, eot_b=27.0):
    b = np.zeros(ctx.hp.n_vocab, np.float32)
    b[ctx.tok.timestamp_begin:] = ts_b
    b[ctx.tok.eot] = eot_b
    return b


def _encode(E, st, ws, win_ctx=None):
    st.set_window_ctx(win_ctx)
    st.mel(_pcm(ws), None, E.OHW_MEL_ZERO_TAIL, want=False)
    st.encode(len(ws))


def _uniforms(E, W, N, cap, seed0=0):
    """candidate j of every window draws from generator seed0 + j, as the engine's candidates do"""
    return np.stack([np.stack([E.HostRng(seed0 + j).uniforms(cap) for j in range(N)]) for _ in range(W)])


def _same(a, b):
    return (a["tokens"] == b["tokens"] and a["ended_by_eot"] == b["ended_by_eot"]
            and np.array_equal(a["logprobs"].view(np.uint32), b["logprobs"].view(np.uint32))
            and np.float32(a["no_speech_prob"]).view(np.uint32) == np.float32(b["no_speech_prob"]).view(np.uint32))


def _ctx(E, tmp_models, dt):
    return E.Context.from_file(tmp_models("micro"), 0, dt)


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("N", [2, 3, 5])
def test_equal_draws_equal_rows_and_permuted_draws_permuted_rows(E, tmp_models, dt, N):
    ctx = _ctx(E, tmp_models, dt)
    W, cap = 2, ctx.hp.n_text_ctx
    st = E.State(ctx, W * N)
    st.set_logit_bias(_bias(ctx))                       # timestamps and end-of-text compete: rows end at different steps
    _encode(E, st, range(W))
    p = ctx.default_params(); p.n_max = N_MAX
    one = E.HostRng(4).uniforms(cap)
    same = st.sample_pass_n(W, N, T_PASS, [1] * W, np.broadcast_to(one, (W, N, cap)).copy(), p)
    for w in range(W):
        for j in range(1, N):
            assert _same(same[w * N], same[w * N + j]), (w, j)
        assert len(same[w * N]["tokens"]) > 0
    u = _uniforms(E, W, N, cap)
    a = st.sample_pass_n(W, N, T_PASS, [1] * W, u, p)
    assert any(a[0]["tokens"] != a[j]["tokens"] for j in range(1, N))          # different draws really give different rows
    perm = list(np.random.default_rng(N).permutation(N))
    if perm == sorted(perm):
        perm = perm[1:] + perm[:1]
    b = st.sample_pass_n(W, N, T_PASS, [1] * W, u[:, perm, :].copy(), p)
    for w in range(W):
        for j in range(N):
            assert _same(b[w * N + j], a[w * N + perm[j]]), (w, j, perm)
    lens = {len(r["tokens"]) + r["ended_by_eot"] for r in a}
    print(f"dt={dt} N={N}: row lengths {sorted(lens)}")


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("N,case", [(2, "text"), (3, "text"), (5, "text"), (3, "audio")])
def test_a_window_in_a_batch_equals_the_window_alone(E, tmp_models, dt, N, case):
    """set_batch_invariant; three windows with text contexts of 0, 5 and 11 tokens (their pasts move to rows w * N), or - case
    "audio" - with unequal window_ctx as well: window w's N rows equal, word for word, the rows of the same window run alone with
    the same N and draws.  A candidate that read another window's cache row, slot or K/V would differ"""
    ctx = _ctx(E, tmp_models, dt)
    W, cap = 3, ctx.hp.n_text_ctx
    rng = np.random.default_rng(21)
    ctxs = [[int(t) for t in rng.integers(0, ctx.tok.eot, size=n)] for n in (0, 5, 11)]
    win_ctx = [1500, 832, 1216] if case == "audio" else None
    p = ctx.default_params(); p.n_max = N_MAX
    u = _uniforms(E, W, N, cap)
    st = E.State(ctx, W * N)
    st.set_batch_invariant(True)
    st.set_logit_bias(_bias(ctx))
    _encode(E, st, range(W), win_ctx)
    st.set_window_prompt(ctxs)
    both = st.sample_pass_n(W, N, 0.4, [1] * W, u, p)            # T < 0.5: the ladder's passes behind a context
    assert np.array_equal(st.fetch("sample_slots", W * N)[:, 0], np.repeat(np.arange(W) * N, N))      # the pasts did move
    st1 = E.State(ctx, N)
    st1.set_batch_invariant(True)
    st1.set_logit_bias(_bias(ctx))
    for w in range(W):
        _encode(E, st1, [w], [win_ctx[w]] if win_ctx else None)
        st1.set_window_prompt([ctxs[w]])
        alone = st1.sample_pass_n(1, N, 0.4, [1], u[w:w + 1], p)
        for j in range(N):
            assert _same(both[w * N + j], alone[j]), (w, j, both[w * N + j]["tokens"], alone[j]["tokens"])
    assert len({tuple(r["tokens"]) for r in both}) > W           # the rows are not all alike


@pytest.mark.parametrize("N", [2, 5])
def test_inactive_window_clean_exit_and_no_second_capture(E, tmp_models, N):
    ctx = _ctx(E, tmp_models, E.OHW_DTYPE_F16)
    W, cap = 3, ctx.hp.n_text_ctx
    st = E.State(ctx, W * N)
    st.set_batch_invariant(True)          # an inactive window changes no variant choice: the active windows' bits must not move
    st.set_logit_bias(_bias(ctx))
    _encode(E, st, range(W))
    p = ctx.default_params(); p.n_max = N_MAX
    before = st.greedy_ex(W, p)
    u = _uniforms(E, W, N, cap)
    full = st.sample_pass_n(W, N, T_PASS, [1, 1, 1], u, p)
    caps = st.counter("step_captures")
    part = st.sample_pass_n(W, N, T_PASS, [1, 0, 1], u, p)
    assert st.counter("step_captures") == caps and st.counter("group_graphs") >= 1      # the same shape: replayed, not captured again
    for j in range(N):
        r = part[N + j]
        assert r["tokens"] == [] and not r["ended_by_eot"] and r["no_speech_prob"] == 0.0 and r["sum_logprob"] == 0.0 and r["logprobs"].size == 0
        assert _same(part[j], full[j]) and _same(part[2 * N + j], full[2 * N + j]), j
    # the entries that follow behave as if the pass had not run
    after = st.greedy_ex(W, p)
    for b in range(W):
        assert _same(before[b], after[b]), b
    act = [1, 0, 1]
    u1 = u[:, 0, :].copy()
    s_before = E.State(ctx, W * N)
    s_before.set_batch_invariant(True)
    s_before.set_logit_bias(_bias(ctx))
    _encode(E, s_before, range(W))
    fresh = s_before.sample_pass(W, T_PASS, act, u1, p)          # a state that never ran a group pass
    mine = st.sample_pass(W, T_PASS, act, u1, p)
    for b in range(W):
        assert _same(fresh[b], mine[b]), b
    if W * 2 <= W * N:
        b1, b2 = s_before.beam_search_ex(W, 2, p), st.beam_search_ex(W, 2, p)
        assert [x["tokens"] for x in b1] == [x["tokens"] for x in b2]
    with pytest.raises(E.WhisperError):
        st.sample_pass_n(W, 6, T_PASS, [1] * W, np.zeros((W, 6, cap)), p)
    with pytest.raises(E.WhisperError):
        E.State(ctx, W * N - 1 if N > 1 else 1).sample_pass_n(W, N, T_PASS, [1] * W, u, p)


@pytest.mark.parametrize("N", [3])
def test_every_candidate_walks_the_oracle(E, oracle, tmp_models, N):
    """f16, three windows, no bias (220 tokens per row) and the timestamp / end-of-text bias: candidate j of window w forced
    through the oracle's decode_pass with MT19937(j), test_gpu_policy's rule per step - a pick may differ only at an edge gap below
    0.02 or a timestamp-rule near-tie - and at least 98 % of all steps identical; log-probabilities within 2 * TOL of the oracle's
    (test_gpu_policy's bound on avg_logprob); the N rows of a window report one no-speech probability, the oracle's within 5 %"""
    from test_gpu_policy import TOL
    path = tmp_models("micro")
    om = oracle.Model.load(path)
    ctx = E.Context.from_file(path, 0, E.OHW_DTYPE_F16)
    W, cap = 3, ctx.hp.n_text_ctx
    st = E.State(ctx, W * N)
    mel = st.mel(_pcm(range(W)), None, E.OHW_MEL_ZERO_TAIL)
    st.encode(W)
    n_steps = n_same = 0
    for bias, n_max in ((None, 60), (_bias(ctx), 220)):
        st.set_logit_bias(bias)
        p = ctx.default_params(); p.n_max = n_max
        op = om.default_params(); op.n_max = n_max
        got = st.sample_pass_n(W, N, T_PASS, [1] * W, _uniforms(E, W, N, cap), p)
        for w in range(W):
            s = oracle.State(om)
            s.set_encoder_output(om.encode(mel[w]))
            for j in range(N):
                g = got[w * N + j]
                toks = g["tokens"] + ([om.tok_eot] if g["ended_by_eot"] else [])
                r = s.decode_pass(op, bias, T_PASS, oracle.MT19937(j), toks)
                assert len(r["choice"]) >= len(toks)
                for i, t in enumerate(toks):
                    n_steps += 1
                    if r["choice"][i] == t:
                        n_same += 1
                        assert abs(float(g["logprobs"][i]) - float(r["plogs"][i])) < 2 * TOL, (w, j, i)
                    else:
                        assert r["gaps"][i] < 0.02 or r["margins"][i] < 2 * TOL / T_PASS, (w, j, i, t, r["choice"][i], float(r["gaps"][i]), float(r["margins"][i]))
                assert abs(g["no_speech_prob"] - r["no_speech_prob"]) < 0.05 * max(r["no_speech_prob"], 1e-6) + 1e-9
                assert g["no_speech_prob"] == got[w * N]["no_speech_prob"]
    st.set_logit_bias(None)
    print(f"best-of pass on the oracle: {n_same} / {n_steps} steps identical")
    assert n_steps > 300 and n_same >= 0.98 * n_steps
