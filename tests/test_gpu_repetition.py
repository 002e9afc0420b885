"""Repetition penalty and no-repeat n-grams through the decoders (ohw_state_set_repeat_rule): the rule inside ohw_greedy_ex,
ohw_sample_pass, ohw_sample_pass_n and ohw_beam_search_ex, and through the engine.  Micro model (f16), 3 windows, n_max 32.

The fixture asserts first that the plain greedy run of every window repeats a text 3-gram inside n_max (the procedural model
settles on one token at once), so the rule has something to stop.
Off means off: rule unset and rule set to (1.0, 0) give the bits of the plain run in all four decoders, launch nothing and
capture nothing.
Against a host loop (fails without the feature): ohw_greedy_ex under (1.3, 3) equals ohw_decode + the numpy rule +
ohw_sample_greedy_host step by step, with and without a hot-phrase table; with the table the loop is also run in the wrong order
(rule first, boost second), which must NOT agree: that fixes boost -> penalty -> ban.
Invariant: under (1.0, 3) no 3-gram that ends in a text token occurs twice in any row any decoder returns.
Graphs: the tokens follow on -> other values -> off -> on; a change of values alone captures nothing.
Engine: lanes and the engine's own state agree, the defaults restore the plain tokens, the host-sampled ladder obeys the rule.
"""
import numpy as np
import pytest

import phrase_ref as P
import repeat_ref as R
from openhush_amd import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N_MAX = 32
SEEDS = (7, 3, 11)
T_PASS = 0.4
DECODERS = ("greedy", "sample", "sample_n", "beam")


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from openhush_amd import engine
    engine.lib()
    return engine


@pytest.fixture(scope="module")
def ctx(E, tmp_models):
    return E.Context.from_file(tmp_models("micro"), 0, E.OHW_DTYPE_F16)


def _encode(E, st, seeds=SEEDS):
    st.mel(np.stack([synth.synth_audio(s) for s in seeds]), None, E.OHW_MEL_REFLECT, want=False)
    st.encode(len(seeds))


def _params(ctx):
    p = ctx.default_params(); p.n_max = N_MAX
    return p


@pytest.fixture(scope="module")
def plain(E, ctx):
    """the plain greedy run of the chosen windows; AHEAD OF EVERYTHING ELSE: each of them repeats a text 3-gram inside n_max"""
    st = E.State(ctx, len(SEEDS))
    _encode(E, st)
    got = st.greedy_ex(len(SEEDS), _params(ctx))
    for w, g in enumerate(got):
        assert R.repeated_ngrams(g["tokens"], 3, ctx.tok.eot), (w, g["tokens"])
    return got


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _same(a, b):
    return (a["tokens"] == b["tokens"] and a["ended_by_eot"] == b["ended_by_eot"] and np.array_equal(_bits(a["logprobs"]), _bits(b["logprobs"]))
            and _bits(a["no_speech_prob"]) == _bits(b["no_speech_prob"]))


def _four_entries(E, st, ctx, K=3):
    """the four decoders on the same windows -> their results, and the repeat_rule tally each of them added"""
    cap = ctx.hp.n_text_ctx
    W = len(SEEDS)
    p = _params(ctx)
    out, tally = {}, {}
    c0 = st.counter("repeat_rule")

    def took(name):
        nonlocal c0
        c1 = st.counter("repeat_rule")
        tally[name] = c1 - c0
        c0 = c1
    _encode(E, st)
    out["greedy"] = st.greedy_ex(W, p); took("greedy")
    out["sample"] = st.sample_pass(W, T_PASS, [1] * W, np.stack([E.HostRng(3 + b).uniforms(cap) for b in range(W)]), p); took("sample")
    u = np.stack([np.stack([E.HostRng(10 * w + j).uniforms(cap) for j in range(3)]) for w in range(W)])
    out["sample_n"] = st.sample_pass_n(W, 3, T_PASS, [1] * W, u, p); took("sample_n")
    out["beam"] = st.beam_search_ex(W, K, p); took("beam")
    return out, tally


def _bias(ctx, ts_b=6.0, eot_b=27.0):
    b = np.zeros(ctx.hp.n_vocab, np.float32)
    b[ctx.tok.timestamp_begin:] = ts_b
    b[ctx.tok.eot] = eot_b
    return b


def _captures(st):
    return st.counter("step_captures"), st.counter("beam_captures")


# ---- off means off -------------------------------------------------------------------------------------------------------
def test_off_means_off(E, ctx, plain):
    """rule unset and rule set to (1.0, 0): tokens, log-probability bits and no-speech bits of the four decoders are the plain
    run's, the tally does not move and no graph is captured.  A bias makes timestamps and end-of-text compete, so rows finish at
    different steps and the done flags matter"""
    st = E.State(ctx, 9)
    st.set_logit_bias(_bias(ctx))
    assert st.repeat_rule() == (1.0, 0)
    base, tally = _four_entries(E, st, ctx)
    assert set(tally.values()) == {0}
    captures = _captures(st)
    st.set_repeat_rule(1.0, 0)
    again, tally = _four_entries(E, st, ctx)
    assert set(tally.values()) == {0} and _captures(st) == captures and st.repeat_rule() == (1.0, 0)
    for name in DECODERS:
        assert len(base[name]) == len(again[name])
        for r in range(len(base[name])):
            assert _same(base[name][r], again[name][r]), (name, r)
    # on, then off again: the plain run's graphs serve, its bits come back
    st.set_repeat_rule(1.3, 3)
    on, tally_on = _four_entries(E, st, ctx)
    assert all(v > 0 for v in tally_on.values()), tally_on
    assert _captures(st)[0] > captures[0] and _captures(st)[1] > captures[1]        # "the rule is on" is part of the graph keys
    assert any(not _same(base["greedy"][r], on["greedy"][r]) for r in range(len(SEEDS)))
    # the first step's history is empty: the no-speech probability is the plain run's
    for name in ("greedy", "sample", "beam"):
        assert all(_bits(base[name][r]["no_speech_prob"]) == _bits(on[name][r]["no_speech_prob"]) for r in range(len(SEEDS))), name
    captures = _captures(st)
    st.set_repeat_rule()
    off, tally = _four_entries(E, st, ctx)
    assert set(tally.values()) == {0} and _captures(st) == captures
    assert all(_same(base[n][r], off[n][r]) for n in DECODERS for r in range(len(base[n])))


# ---- against a host loop -------------------------------------------------------------------------------------------------
def _host_loop(ctx, st, p, B, modify):
    """ohw_decode + modify(row, history) + ohw_sample_greedy_host, step by step, on the device's own logits -> (tokens, logprobs)"""
    prompt = [ctx.tok.sot, ctx.tok.sot + 1 + p.lang_id, ctx.tok.transcribe]
    logits = st.decode(np.tile(np.asarray(prompt, np.int32), (B, 1)), [0] * B)
    out, lps = [[] for _ in range(B)], [[] for _ in range(B)]
    done, n_past, feed = [False] * B, [len(prompt)] * B, [0] * B
    for _ in range(N_MAX):
        for b in range(B):
            if done[b]:
                continue
            tok, lp = ctx.sample_greedy_host(p, modify(logits[b], out[b]), out[b])
            lps[b].append(lp)
            if tok == ctx.tok.eot:
                done[b] = True
                continue
            out[b].append(tok)
            feed[b] = tok
            done[b] = len(out[b]) >= N_MAX
        if all(done):
            break
        logits = st.decode(np.asarray(feed, np.int32).reshape(B, 1), n_past)
        n_past = [n + (0 if done[b] else 1) for b, n in enumerate(n_past)]
    return out, lps


@pytest.mark.parametrize("with_table", [False, True], ids=["rule_alone", "behind_a_phrase_table"])
def test_greedy_equals_a_host_loop_with_the_numpy_rule(E, ctx, plain, with_table):
    """ohw_greedy_ex under (1.3, 3) == a loop of ohw_decode, the numpy rules and ohw_sample_greedy_host: the tokens exactly (the
    loop works on the device's own logits), the log-probabilities within 2e-4, the bound test_gpu_sampler.py holds the device
    sampler to against the host's.  The table (8 phrases at boost 2.0 over the model's favourite tokens) raises tokens the
    penalty then scales: in the order penalty -> ban -> boost the loop's log-probabilities move by tenths (0.4 on the float32
    oracle), so the same comparison tells the orders apart"""
    theta, n = 1.3, 3
    eot = ctx.tok.eot
    B = len(SEEDS)
    rng = np.random.default_rng(17)
    top = [47018, 17019, 20198, 8911, 11308]
    phrases = [[int(t) for t in rng.choice(top, size=int(rng.integers(2, 5)))] for _ in range(8)]
    table = P.build(phrases, [2.0] * 8)
    st = E.State(ctx, B)
    _encode(E, st)
    p = _params(ctx)
    st.set_repeat_rule(theta, n)
    if with_table:
        st.set_phrase_table(phrases, 2.0)
    got = st.greedy_ex(B, p)
    assert st.counter("repeat_rule") > 0
    assert [g["tokens"] for g in got] != [g["tokens"] for g in plain]              # the rule changed the decode
    st.set_repeat_rule()
    st.set_phrase_table(None)

    def hist(h):
        return np.asarray(h + [0], np.int32)

    def right(row, h):
        if with_table:
            row = P.boost(table, hist(h), len(h), row)
        return R.rule(theta, n, hist(h), len(h), row, eot)

    def wrong(row, h):
        row = R.rule(theta, n, hist(h), len(h), row, eot)
        return P.boost(table, hist(h), len(h), row)
    out, lps = _host_loop(ctx, st, p, B, right)
    for b in range(B):
        assert got[b]["tokens"] == out[b], b
        assert np.abs(got[b]["logprobs"] - np.asarray(lps[b], np.float32)).max() < 2e-4, b
        assert not R.repeated_ngrams(out[b], n, eot)
    if with_table:
        out_w, lps_w = _host_loop(ctx, st, p, B, wrong)
        far = [out_w[b] != out[b] or np.abs(np.asarray(lps_w[b]) - np.asarray(lps[b])).max() > 0.05 for b in range(B)]
        assert all(far), far


# ---- the invariant -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("biased", [False, True], ids=["plain_rows", "timestamps_and_eot_compete"])
def test_no_text_3gram_twice_in_any_row_of_any_decoder(E, ctx, plain, biased):
    """(1.0, 3): by construction, for any draw - greedy, the temperature pass at T = 0.4, 3 candidates per window, 5 beams"""
    eot = ctx.tok.eot
    st = E.State(ctx, 15)
    if biased:
        st.set_logit_bias(_bias(ctx))
    st.set_repeat_rule(1.0, 3)
    out, tally = _four_entries(E, st, ctx, K=5)
    assert all(v > 0 for v in tally.values()), tally
    assert len(out["sample_n"]) == 3 * len(SEEDS) and len(out["beam"]) == len(SEEDS)
    n_rows = 0
    for name in DECODERS:
        for r, g in enumerate(out[name]):
            assert R.repeated_ngrams(g["tokens"], 3, eot) == [], (name, r, g["tokens"])
            assert len(g["tokens"]) >= 3 or g["ended_by_eot"], (name, r)
            n_rows += 1
    assert n_rows == 3 + 3 + 9 + 3
    if not biased:
        # the rule was needed: the plain greedy rows repeat (the fixture), these do not, and nothing was cut short
        assert all(len(g["tokens"]) == N_MAX for g in out["greedy"])


# ---- graphs ----------------------------------------------------------------------------------------------------------------
def test_tokens_follow_the_setting_and_new_values_capture_nothing(E, ctx, plain):
    st = E.State(ctx, 1)
    _encode(E, st, SEEDS[:1])
    p = _params(ctx)
    eot = ctx.tok.eot
    run = lambda: st.greedy_ex(1, p)[0]["tokens"]
    assert run() == plain[0]["tokens"]
    c_plain = _captures(st)
    st.set_repeat_rule(1.0, 3)
    on3 = run()
    c_on = _captures(st)
    assert c_on[0] == c_plain[0] + 1 and not R.repeated_ngrams(on3, 3, eot) and R.repeated_ngrams(on3, 2, eot)
    st.set_repeat_rule(1.0, 2)                             # other values on the same buffer: the captured step serves
    on2 = run()
    assert _captures(st) == c_on and not R.repeated_ngrams(on2, 2, eot) and on2 != on3
    st.set_repeat_rule(2.0, 0)
    pen = run()
    assert _captures(st) == c_on and pen not in (on2, on3, plain[0]["tokens"])
    st.set_repeat_rule(1.0, 0)
    assert run() == plain[0]["tokens"] and _captures(st) == c_on
    st.set_repeat_rule(1.0, 3)
    assert run() == on3 and _captures(st) == c_on


# ---- engine ----------------------------------------------------------------------------------------------------------------
def _windows(eng):
    """the kept tokens of the last transcribe, per window"""
    toks, out, i = eng.last_tokens(), [], 0
    for q in eng.last_quality_ex():
        out.append(toks[i:i + q["n_tokens"]])
        i += q["n_tokens"]
    assert i == len(toks)
    return out


def test_engine_repetition_on_lanes_and_on_its_own_state(E, tmp_models):
    path = tmp_models("micro")
    pcm = np.concatenate([synth.synth_audio(40 + w) for w in range(3)])[:16000 * 70]

    def run(schedule, setting):
        eng = E.WhisperEngine.new(path, "en", False, True, 0, E.OHW_DTYPE_F16, 1)
        eng.set_decode_policy(temperature_inc=0.0)
        E.lib().ohw_engine_set_force_len(eng.h, 16)
        eng.set_schedule(schedule, lanes=2, merge=1)
        if setting:
            eng.set_repetition(*setting)
        eng.transcribe(E.AudioBuffer(pcm.copy(), 16000))
        wins = _windows(eng)
        eng.set_repetition()
        eng.transcribe(E.AudioBuffer(pcm.copy(), 16000))
        cleared = _windows(eng)
        eng.close()
        return wins, cleared
    plain, _ = run(E.OHW_SCHEDULE_SEQUENTIAL, None)
    own, own_cleared = run(E.OHW_SCHEDULE_SEQUENTIAL, (1.3, 3))
    lanes, lanes_cleared = run(E.OHW_SCHEDULE_LANES, (1.3, 3))
    eot = 50257
    assert len(plain) == 3 and all(R.repeated_ngrams(w, 3, eot) for w in plain)
    assert own == lanes and own != plain and all(not R.repeated_ngrams(w, 3, eot) for w in own)
    assert own_cleared == plain and lanes_cleared == plain
    with pytest.raises(E.WhisperError):
        eng = E.WhisperEngine.new(path, "en", False, True, 0, E.OHW_DTYPE_F16, 1)
        try:
            eng.set_repetition(0.001, 3)
        finally:
            eng.close()


def test_host_sampled_ladder_obeys_the_rule(E, tmp_models):
    """logprob_thold 0 rejects every pass, so each window climbs the whole ladder on the host; every pass of the trace and the
    kept tokens hold no text 3-gram twice under (1.0, 3), and without the rule the T = 0 pass does"""
    path = tmp_models("micro")
    pcm = np.concatenate([synth.synth_audio(40 + w) for w in range(2)])
    eot = 50257
    eng = E.WhisperEngine.new(path, "en", False, True, 0, E.OHW_DTYPE_F16, 2)
    eng.set_decode_policy(logprob_thold=0.0)
    E.lib().ohw_engine_set_force_len(eng.h, 16)
    eng.transcribe(E.AudioBuffer(pcm.copy(), 16000))
    trace = eng.last_trace()
    assert any(R.repeated_ngrams(t, 3, eot) for _, T, t in trace if T == 0.0)
    eng.set_repetition(1.0, 3)
    eng.transcribe(E.AudioBuffer(pcm.copy(), 16000))
    trace = eng.last_trace()
    temps = sorted({round(T, 1) for _, T, _ in trace})
    assert temps[0] == 0.0 and temps[-1] >= 0.8 and len(trace) >= 2 * len(temps)
    for w, T, toks in trace:
        assert R.repeated_ngrams(toks, 3, eot) == [], (w, T, toks)
    kept = _windows(eng)
    assert len(kept) == 2 and all(len(k) >= 3 and not R.repeated_ngrams(k, 3, eot) for k in kept)
    assert all(q["temperature"] > 0.0 for q in eng.last_quality_ex())                 # the kept pass came from the ladder
    eng.close()
