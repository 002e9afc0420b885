"""The temperature fallback sampled on the device (ohw_sample_pass, ohw_engine_set_fallback_device) against the host ladder
(ohw_sample_host) and the oracle.

The host keeps whisper.cpp's std::mt19937 generators and hands the device each pass's draws in advance (ohw_rng_uniforms);
the device picks the first index whose partial sum of probabilities reaches u * their total, std::discrete_distribution's
lower bound up to rounding.  So a pick may differ from the host's only where the draw lies next to an interval edge of the
host's cumulative distribution (or, at f16 logits, where the timestamp-mass rule is a near-tie); everything else -
passes, temperatures, decisions, kept tokens - is checked like the host ladder in test_gpu_policy."""
import ctypes as C
import os
import time

import numpy as np
import pytest

from openhush_amd import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# observed on MI355X (printed by the tests), the tolerances twice that:
KERNEL_LP_TOL = 1.6e-5        # log-probability of the same pick, device (float lse) against the host (double lse): 7.6e-6
KERNEL_NSP_TOL = 3.4e-6        # no-speech probability of a first step, absolute: 1.67e-6
KERNEL_EDGE_GAP = 1e-5        # a different pick only where the host's draw is this close to an interval edge (none seen)
LARGE_V3_SAME = 0.95          # share of oracle-identical steps, large-v3 f16 window through six passes: 0.974 observed


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


def _bias(om, ts_b, eot_b):
    b = np.zeros(om.n_vocab, np.float32)
    b[om.tok_beg:] = ts_b
    b[om.tok_eot] = eot_b
    return b


def _host_edge_gap(p: np.ndarray, u: float) -> float:
    """distance of u to the nearer edge of the interval std::discrete_distribution picks over probabilities p"""
    pd = p.astype(np.float64)
    cp = np.cumsum(pd / pd.sum())
    cp[-1] = 1.0
    k = int(np.searchsorted(cp, u, side="left"))
    left = cp[k - 1] if k > 0 else 0.0
    return float(min(u - left, cp[k] - u))


def _host_probs(E, ctx, p, row, hist, T, bias):
    """what ohw_sample_host hands std::discrete_distribution: float32 exp(v - lse) over the filtered row v = (row + bias) / T
    (ohw_sample_greedy_host applies the same filter in place and returns logits[best] - lse)"""
    f = ((row + (bias if bias is not None else 0)).astype(np.float32) / np.float32(T)).astype(np.float32)
    c = np.asarray(hist or [0], np.int32)
    lp = C.c_float(0)
    tok = E.lib().ohw_sample_greedy_host(ctx.h, C.byref(p), E._fp(f), E._ip(c), len(hist), C.byref(lp))
    lse = np.float32(f[tok] - np.float32(lp.value))
    return np.where(f == -np.inf, np.float32(0), np.exp((f - lse).astype(np.float32))).astype(np.float32)


def test_predrawn_lower_bound_matches_the_host_sampler_draw_for_draw(E, oracle):
    """ohw_sample_host sharing ONE generator against the pre-drawn path (ohw_rng_uniforms of another generator, the lower
    bound in host code over ohw_sample_host's own probabilities, ohw_rng_discard_draws(1) per step), on the sampler goldens'
    rows at T = 0.2, 0.6 and 1.0, with and without history: the same token every time (the host's context needs a device)."""
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "sampler.npz"))
    rows = g["rows_f16"].astype(np.float32)
    hists = [[int(t) for t in g["hists"][g["hist_of_row"][r]] if t >= 0] for r in range(rows.shape[0])]
    hp = synth.PRESETS["nano"]
    ctx = E.Context.synthetic(hp.as_list(), 1234, 0, E.OHW_DTYPE_F16)
    p = ctx.default_params()
    rng, pre = E.HostRng(0), E.HostRng(0)
    n = 0
    for T in (0.2, 0.6, 1.0):
        for r in range(rows.shape[0]):
            for hist in ([], hists[r]) if hists[r] else ([],):
                tok, _, _ = ctx.sample_host(p, rows[r], hist, T, rng)
                u = pre.uniforms(1)[0]
                pre.discard_draws(1)
                probs = _host_probs(E, ctx, p, rows[r], hist, T, None)
                pd = probs.astype(np.float64)
                cp = np.cumsum(pd / pd.sum()); cp[-1] = 1.0
                mine = int(np.searchsorted(cp, u, side="left"))
                assert mine == tok or _host_edge_gap(probs, u) < 1e-9, (T, r, len(hist), mine, tok)
                n += 1
    assert n > 40
    assert pre.uniforms(4).tobytes() == rng.uniforms(4).tobytes()          # both generators at the same place


def test_temperature_kernel_against_the_host_sampler(E, oracle):
    """ohw_dbg_sample_t (the device temperature sampler) against ohw_sample_host on the golden rows: three temperatures,
    with and without a logit bias, every row once as a window's first step (no history) and once with its history."""
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "sampler.npz"))
    rows = g["rows_f16"].astype(np.float32)
    hists = [[int(t) for t in g["hists"][g["hist_of_row"][r]] if t >= 0] for r in range(rows.shape[0])]
    hp = synth.PRESETS["nano"]
    ctx = E.Context.synthetic(hp.as_list(), 1234, 0, E.OHW_DTYPE_F16)
    om = oracle.Model.synth(hp.as_list(), 1234)
    R = rows.shape[0]
    # plus first steps with real no-speech mass (the goldens' rows give it ~0): the no-speech logit near the row's maximum
    ns_rows = []
    for k, d in enumerate((-1.0, 0.5, 2.0)):
        x = rows[k].copy()
        x[ctx.tok.nosp] = x.max() + d
        ns_rows.append(x)
    allrows = np.concatenate([rows, rows, np.stack(ns_rows)])
    allh = [[] for _ in range(R)] + hists + [[] for _ in ns_rows]
    NR = allrows.shape[0]
    st = E.State(ctx, NR)
    p = ctx.default_params()
    rng = np.random.default_rng(5)
    worst_lp = worst_nsp = max_nsp = 0.0
    n = same = 0
    edge = []
    for use_bias in (False, True):
        bias = None
        if use_bias:
            bias = (rng.standard_normal(hp.n_vocab) * 1.5).astype(np.float32)
            bias[om.tok_beg:] += 4.0
        st.set_logit_bias(bias)
        for T in (0.2, 0.6, 1.0):
            gen = E.HostRng(17 + int(T * 10) + 100 * use_bias)
            u = gen.uniforms(NR)
            tok, lp, nsp = st.dbg_sample_t(p, allrows, allh, T, u)
            for r in range(NR):
                row = allrows[r] + (bias if use_bias else 0)
                # the host sampler with a generator positioned at this row's draw
                gen_r = E.HostRng(17 + int(T * 10) + 100 * use_bias)
                gen_r.discard_draws(r)
                ht, hlp, hns = ctx.sample_host(p, row.copy(), allh[r], T, gen_r)
                n += 1
                if int(tok[r]) == ht:
                    same += 1
                    worst_lp = max(worst_lp, abs(float(lp[r]) - hlp))
                    assert abs(float(lp[r]) - hlp) < KERNEL_LP_TOL, (use_bias, T, r, float(lp[r]), hlp)
                else:
                    gap = _host_edge_gap(_host_probs(E, ctx, p, allrows[r], allh[r], T, bias), float(u[r]))
                    edge.append(gap)
                    assert gap < KERNEL_EDGE_GAP, (use_bias, T, r, int(tok[r]), ht, gap)
                if not allh[r]:
                    worst_nsp = max(worst_nsp, abs(float(nsp[r]) - hns))
                    max_nsp = max(max_nsp, hns)
                    assert abs(float(nsp[r]) - hns) < KERNEL_NSP_TOL, (use_bias, T, r, float(nsp[r]), hns)
    print(f"temperature kernel: {same} / {n} picks identical; edge gaps of the others {edge}; worst |dlogprob| {worst_lp:.2e}; "
          f"worst |d no-speech| {worst_nsp:.2e} (no-speech probabilities up to {max_nsp:.3f})")
    assert max_nsp > 0.3                        # the no-speech rows really carry mass
    assert same >= n - 2
    # the T = 0 sampler is untouched by a temperature launch on the same state
    st.set_logit_bias(None)
    t0, _, _ = st.dbg_sample(p, rows, hists)
    assert [int(x) for x in t0] == [int(x) for x in g["argmax"]]


def _walk(E, oracle, om, eng, wins, bias, pol, **kw):
    from test_gpu_policy import _walk_and_compare
    return _walk_and_compare(E, oracle, om, eng, wins, bias, pol, **kw)


def _trace_passes(trace):
    return [(w, round(T, 3), list(t)) for w, T, t in trace]


def test_device_ladder_matches_oracle_pass_by_pass_and_the_host_ladder(E, oracle, tmp_models):
    """test_temperature_ladder_matches_oracle_pass_by_pass's setup through the device ladder: micro, f16, three windows in one
    batch, no bias (every window runs all six passes) and the timestamp / end-of-text bias.  Every pass is walked on the
    oracle (edge gap < 0.02 or a timestamp-rule near-tie; >= 98 % of steps identical); a second transcribe gives the same
    text; the host ladder gives the same trace except at draws next to an interval edge."""
    path = tmp_models("micro")
    om = oracle.Model.load(path)
    pcm = np.concatenate([synth.synth_audio(7), synth.synth_audio(3), synth.synth_audio(11, 200000)])
    wins = [pcm[0:480000], pcm[480000:960000], pcm[960000:]]
    pol = oracle.default_policy()
    total = [0, 0, 0]
    for bias in (None, _bias(om, 6.0, 27.0)):
        traces = {}
        for dev in (False, True):
            eng = E.WhisperEngine.new(path, "auto", False, True, 0, E.OHW_DTYPE_F16, 3)
            eng.set_fallback_on_device(dev)
            if bias is not None:
                E.lib().ohw_state_set_logit_bias(E.lib().ohw_engine_state(eng.h), bias.ctypes.data_as(C.POINTER(C.c_float)), bias.size)
            res = eng.transcribe(E.AudioBuffer(pcm, 16000))
            traces[dev] = _trace_passes(eng.last_trace())
            if dev:
                n_pass, n_steps, n_same = _walk(E, oracle, om, eng, wins, bias, pol)
                print(f"device ladder: bias={'yes' if bias is not None else 'no'}: {n_pass} passes, {n_same} / {n_steps} steps identical; "
                      f"temperatures kept {[round(q['temperature'], 1) for q in eng.last_quality_ex()]}")
                total = [a + b for a, b in zip(total, (n_pass, n_steps, n_same))]
                if bias is None:
                    assert n_pass == 18 and all(abs(q["temperature"] - 1.0) < 1e-3 for q in eng.last_quality_ex())
                again = eng.transcribe(E.AudioBuffer(pcm, 16000))
                assert again.text == res.text
            eng.close()
        # host ladder against device ladder, window by window: the same passes and tokens.  Both sample the same device
        # logits from the same generators; a pick may differ only at a draw within ~1e-5 of an interval edge (the kernel
        # test's class, about one step in 10^5 here), after which that window's passes go their own way
        def by_win(tr):
            d = {}
            for w, T, t in tr:
                d.setdefault(w, []).append((T, t))
            return d
        hw, dw = by_win(traces[False]), by_win(traces[True])
        assert sorted(hw) == sorted(dw)
        differ = [w for w in hw if hw[w] != dw[w]]
        print(f"host vs device ladder (bias={'yes' if bias is not None else 'no'}): {len(traces[False])} / {len(traces[True])} passes, "
              f"windows that differ: {differ}")
        assert len(differ) <= 1
    assert total[2] >= 0.98 * total[1]


def test_device_ladder_seek_mode_shared_generator(E, oracle, tmp_models):
    """test_seek_loop_with_timestamps_matches_oracle's case through the device ladder: one generator for the whole call,
    advanced by exactly the draws each kept pass consumed, windows advanced by their last timestamp."""
    path = tmp_models("micro")
    om = oracle.Model.load(path)
    bias = _bias(om, 8.0, 26.0)
    pcm = np.concatenate([synth.synth_audio(41), 0.1 * synth.synth_audio(42, 200000)]).astype(np.float32)
    eng = E.WhisperEngine.new(path, "en", False, True, 0, E.OHW_DTYPE_F16, 1)
    eng.set_window_mode(E.OHW_WINDOW_SEEK)
    eng.set_fallback_on_device(True)
    E.lib().ohw_state_set_logit_bias(E.lib().ohw_engine_state(eng.h), bias.ctypes.data_as(C.POINTER(C.c_float)), bias.size)
    pol = oracle.default_policy()
    eng.transcribe(E.AudioBuffer(pcm, 16000))
    q = eng.last_quality_ex()
    seek_end = oracle.mel_frames(len(pcm))
    seeks, wins = [], []
    seek = 0
    for x in q:
        seeks.append(seek)
        wins.append(pcm[seek * 160: seek * 160 + 480000])
        seek += x["seek_delta"] if x["seek_delta"] > 0 else 3000
    assert seek + 100 >= seek_end and len(q) >= 2
    assert any(x["seek_delta"] != 3000 for x in q)
    n_fallback = sum(1 for x in q if x["temperature"] > 0)
    rec_max = om.recording_max(pcm)
    mels = [om.log_mel_seek(pcm, sk, rec_max) for sk in seeks]
    n_pass, n_steps, n_same = _walk(E, oracle, om, eng, wins, bias, pol, seeks=seeks, ends=[seek_end] * len(q), mode=1, mels=mels)
    print(f"seek loop, device ladder: {len(q)} windows, {n_fallback} kept a T > 0 pass, seek deltas {[x['seek_delta'] for x in q]}, "
          f"{n_pass} passes, {n_same} / {n_steps} steps identical")
    assert n_same >= 0.98 * n_steps
    eng.close()


def test_device_ladder_at_large_v3_dims_with_lanes(E, oracle, tmp_models):
    """large-v3 dims, f16, 3 windows with max_batch 2 (two decode batches: the LANES schedule, one lane thread each), the
    default policy, the device ladder.  Unbiased procedural weights: every window fails through the repetition guard and runs
    all six passes.  Every kept pass's temperature is on the ladder, the decisions agree with the oracle's rules on the
    returned tokens, and window 0 is walked on the oracle through all its passes: every step within the edge / near-tie
    tolerance of test_gpu_policy, and at least LARGE_V3_SAME of them identical outright (32 f16 layers drift further from the
    oracle than micro's 2).  Bounded: the transcribe asserts its own time (4 s observed, 120 s allowed); the oracle's walk on
    the CPU takes about a minute."""
    path = tmp_models("large-v3")
    pcm = np.concatenate([synth.synth_audio(1000 + w) for w in range(3)])
    eng = E.WhisperEngine.new(path, "auto", False, True, 0, E.OHW_DTYPE_F16, 2)
    eng.set_schedule(E.OHW_SCHEDULE_LANES, 2, 1)
    eng.set_fallback_on_device(True)
    t0 = time.perf_counter()
    eng.transcribe(E.AudioBuffer(pcm, 16000))
    dt = time.perf_counter() - t0
    trace = eng.last_trace()
    q = eng.last_quality_ex()
    print(f"large-v3 device ladder: 3 windows, {len(trace)} passes in {dt:.2f} s (LANES, 2 lanes)")
    assert dt < 120.0
    ladder = [0.0, 0.2, 0.4, 0.6, 0.8, 1.0]
    om = oracle.Model.load(path)
    pol = oracle.default_policy()
    by_win = {}
    for w, T, toks in trace:
        by_win.setdefault(w, []).append((T, toks))
    assert sorted(by_win) == [0, 1, 2]
    for w, passes in by_win.items():
        assert [round(T, 3) for T, _ in passes] == ladder[:len(passes)]
        assert any(abs(q[w]["temperature"] - x) < 1e-3 for x in ladder)
        assert abs(q[w]["temperature"] - passes[-1][0]) < 1e-3
    # window 0 through all its passes on the oracle (f16: the tolerances of test_gpu_policy)
    p = om.default_params()
    s = oracle.State(om)
    s.set_encoder_output(om.encode(om.log_mel(pcm[:480000], 1)))
    rng = oracle.MT19937(0)
    n_steps = n_same = 0
    passes = by_win[0]
    t1 = time.perf_counter()
    for k, (T, toks) in enumerate(passes):
        r = s.decode_pass(p, None, T, rng, toks)
        for i, t in enumerate(toks):
            n_steps += 1
            if r["choice"][i] == t:
                n_same += 1
            elif T == 0.0:
                assert r["margins"][i] < 0.06, (k, i)
            else:
                assert r["gaps"][i] < 0.02 or r["margins"][i] < 0.06 / T, (k, i, float(r["gaps"][i]), float(r["margins"][i]))
        ev = oracle.evaluate_sequence(om, toks, r["plogs"], 0, 2999, 220, False, 0)
        assert ev.n_sampled == len(toks)
        assert oracle.pass_needs_fallback(ev, pol, r["no_speech_prob"], k == len(ladder) - 1) == (k + 1 < len(passes)), (k, ev.as_dict())
    print(f"large-v3 window 0: {len(passes)} passes, {n_same} / {n_steps} steps identical on the oracle ({time.perf_counter() - t1:.1f} s)")
    assert n_same >= LARGE_V3_SAME * n_steps
    eng.close()


def test_pool_fallback_device_equals_one_engine(E, tmp_models):
    """ohw_pool_set_fallback_device: device 0 listed twice gives the single engine's tokens with the device ladder on.  One
    window per batch and the sequential schedule on both sides: every engine decodes more than one batch, so all run the
    batch-invariant kernel variants (a T > 0 draw sees every bit of the logits, an arg-max does not)."""
    path = tmp_models("micro")
    pcm = np.concatenate([synth.synth_audio(70 + w) for w in range(3)] + [synth.synth_audio(75, 90000)])
    eng = E.WhisperEngine.new(path, "auto", False, True, 0, E.OHW_DTYPE_F16, 1)
    eng.set_schedule(E.OHW_SCHEDULE_SEQUENTIAL)
    eng.set_fallback_on_device(True)
    ref = eng.transcribe(E.AudioBuffer(pcm, 16000))
    ref_tokens, ref_temps = eng.last_tokens(), [round(x["temperature"], 3) for x in eng.last_quality_ex()]
    eng.close()
    assert any(t > 0 for t in ref_temps)                      # the ladder really ran
    pool = E.EnginePool(path, "auto", False, [0, 0], E.OHW_DTYPE_F16, 1)
    pool.set_schedule(E.OHW_SCHEDULE_SEQUENTIAL)
    pool.set_fallback_on_device(True)
    res = pool.transcribe(E.AudioBuffer(pcm, 16000))
    assert res.text == ref.text and pool.last_tokens() == ref_tokens
    pool.close()
