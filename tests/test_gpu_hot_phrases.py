"""Hot phrases through the decoders (ohw_state_set_phrase_table): the history-dependent boost inside ohw_greedy_ex,
ohw_sample_pass, ohw_sample_pass_n and ohw_beam_search_ex, and through the engine.  Micro model (f16), at most 3 windows, n_max 24.

Off means off: no table, an empty table and a table of zero boosts give the bits of the plain run.
Forced cycle (fails without the feature): two windows decode under a table of two phrases whose boosts are twice the spread of
the oracle's logits, so every step is decided by the table and by margins the fixture checks on the oracle first:
  window 0 must emit P = (p0, p1, p2) over and over: inside the phrase the node [p0] / [p0, p1] raises the continuation, which
      beats the root's p0 and q0 by its natural logit (p1, p2 are two of the model's favourite tokens); behind p2 nothing but
      the root matches and p0 beats q0;
  window 1 must emit (q0, q1) over and over: the second phrase is q0 q1 q0 q1 ... (16 tokens), so behind its first token the
      nested matches of every even (odd) depth pile their boosts on q1 (q0) and the history never holds p0.
  Which of p0 and q0 a window starts with is the one decision the audio takes: p0 and q0 are the text tokens whose step-0 logit
  difference between the two windows is largest (found by a search over the oracle's rows for synthetic windows 11 and 5), and
  the second boost sits in the middle of the gap.  The fixture asserts every margin on the oracle before the GPU is asked.
Against a host loop: ohw_greedy_ex under a table equals ohw_decode + the numpy rule + ohw_sample_greedy_host.
Engine: lanes and the engine's own state agree, clearing restores the plain tokens.
"""
import numpy as np
import pytest

import phrase_ref as R
from openhush_amd import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N_MAX = 24
SEEDS = (11, 5)                                  # the synthetic windows of the forced cycle
P = [41949, 47018, 17019]                        # p0 from the search, then the model's two favourite text tokens
Q0, Q1 = 21348, 8911                             # q0 from the search; q1: the model's favourite text token behind q0
Q = [Q0, Q1] * 8
MARGIN = 2.0          # every decision of the forced cycle, on the oracle: 60 times the f16 logit tolerance of test_gpu_parity (0.03)
T_PASS = 0.4
# a draw inside [0.05, 0.95] picks any token that holds more than 95 % of the mass; at MARGIN the rivals hold exp(-MARGIN / T) = 0.7 %
U_LO, U_HI = 0.05, 0.95


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
def ctx(E, tmp_models):
    return E.Context.from_file(tmp_models("micro"), 0, E.OHW_DTYPE_F16)


def _pcm(seeds):
    return np.stack([synth.synth_audio(s) for s in seeds])


def _encode(E, st, seeds):
    st.mel(_pcm(seeds), None, E.OHW_MEL_REFLECT, want=False)
    st.encode(len(seeds))


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _same(a, b):
    return (a["tokens"] == b["tokens"] and a["ended_by_eot"] == b["ended_by_eot"] and np.array_equal(_bits(a["logprobs"]), _bits(b["logprobs"]))
            and _bits(a["no_speech_prob"]) == _bits(b["no_speech_prob"]))


def _uniforms(E, shape_rows, cap):
    u = np.stack([E.HostRng(r).uniforms(cap) for r in range(shape_rows)])
    return np.clip(u, U_LO, U_HI)


@pytest.fixture(scope="module")
def plans(oracle, tmp_models):
    """no_timestamps -> the plan under that prompt (the no-timestamps token is part of the prompt, so the rows differ)"""
    om = oracle.Model.load(tmp_models("micro"))
    return {nts: _plan(oracle, om, nts) for nts in (0, 1)}


@pytest.fixture(scope="module")
def plan(plans):
    return plans[0]


def _plan(oracle, om, no_timestamps):
    """the forced cycle, planned on the oracle once: the expected tokens of both windows, the table, and the proof that every step
    of both windows is decided with MARGIN to spare"""
    op = om.default_params()
    op.no_timestamps = no_timestamps
    prompt = om.build_prompt(op)
    want = [(P * 8)[:N_MAX], (Q * 2)[:N_MAX]]
    assert len(set(P)) == 3 and om.tok_blank not in P + Q and max(P + Q) < om.tok_eot and Q0 not in P and P[0] not in Q
    rows = []
    for w, seed in enumerate(SEEDS):
        s = oracle.State(om)
        s.set_encoder_output(om.encode(om.log_mel(synth.synth_audio(seed), 0)))
        r = [s.decode(prompt, 0)]
        for i in range(N_MAX - 1):
            r.append(s.decode([want[w][i]], len(prompt) + i))
        rows.append(np.stack(r))
    spread = max(float(r.max() - r.min()) for r in rows)
    floor = 2.0 * spread                          # both boosts are at least this
    # p0 against q0 where only the root matches: window 0 at its restarts, window 1 at its first step
    upper = float((rows[0][::3, P[0]] - rows[0][::3, Q0]).min())
    lower = float(rows[1][0, P[0]] - rows[1][0, Q0])
    assert upper - lower > 2 * MARGIN, (lower, upper)
    mid = 0.5 * (upper + lower)                   # boost_q - boost_p sits in the middle of the gap
    boost_p, boost_q = (floor - mid, floor) if mid < 0 else (floor, floor + mid)
    phrases, boosts = [P, Q], [boost_p, boost_q]
    table = R.build(phrases, boosts)
    margins = []
    for w in range(2):
        for i in range(N_MAX):
            row = R.boost(table, np.asarray(want[w] + [0], np.int32), i, rows[w][i])
            top = int(row.argmax())
            rest = np.delete(row, top).max()
            assert top == want[w][i], (w, i, top)
            margins.append(float(row[top] - rest))
    assert min(margins) >= MARGIN, min(margins)
    print(f"forced cycle (no_timestamps {no_timestamps}, prompt of {len(prompt)}): spread {spread:.2f}, boosts {boost_p:.2f} / {boost_q:.2f}, smallest margin on the oracle {min(margins):.2f}")
    return {"want": want, "phrases": phrases, "boosts": boosts, "spread": spread}


# ---- off means off -------------------------------------------------------------------------------------------------------
def _four_entries(E, st, ctx, seeds):
    """the four decoders on the same windows -> their results, and the phrase_boost tally each of them added"""
    cap = ctx.hp.n_text_ctx
    W = len(seeds)
    p = ctx.default_params(); p.n_max = N_MAX
    out, tally = {}, {}
    c0 = st.counter("phrase_boost")

    def took(name):
        nonlocal c0
        c1 = st.counter("phrase_boost")
        tally[name] = c1 - c0
        c0 = c1
    _encode(E, st, seeds)
    out["greedy"] = st.greedy_ex(W, p); took("greedy")
    out["sample"] = st.sample_pass(W, 0.6, [1] * W, np.stack([E.HostRng(3 + b).uniforms(cap) for b in range(W)]), p); took("sample")
    u = np.stack([np.stack([E.HostRng(j).uniforms(cap) for j in range(3)]) for _ in range(W)])
    out["sample_n"] = st.sample_pass_n(W, 3, 0.6, [1] * W, u, p); took("sample_n")
    out["beam"] = st.beam_search_ex(W, 3, p); took("beam")
    return out, tally


def _bias(ctx, ts_b=6.0, eot_b=27.0):
    b = np.zeros(ctx.hp.n_vocab, np.float32)
    b[ctx.tok.timestamp_begin:] = ts_b
    b[ctx.tok.eot] = eot_b
    return b


def test_off_means_off(E, ctx):
    """no table, an empty table and all boosts 0.0: tokens, log-probabilities and no-speech probabilities of the four entries are
    the no-table run's bits; the tally is 0 without a table and positive with one, in each entry.  A bias makes timestamps and
    end-of-text compete, so rows finish at different steps and the done flags matter"""
    seeds = (7, 3)
    st = E.State(ctx, 6)
    st.set_logit_bias(_bias(ctx))
    base, tally = _four_entries(E, st, ctx, seeds)
    assert tally == {"greedy": 0, "sample": 0, "sample_n": 0, "beam": 0} and st.phrase_count() == 0
    st.set_phrase_table([])
    again, tally = _four_entries(E, st, ctx, seeds)
    assert tally == {"greedy": 0, "sample": 0, "sample_n": 0, "beam": 0} and st.phrase_count() == 0
    captures = st.counter("step_captures"), st.counter("beam_captures")
    top = [47018, 17019, 20198, 8911]
    st.set_phrase_table([top[:3], top[1:], [top[3], top[0]], [ctx.tok.blank]], 0.0)
    assert st.phrase_count() == 4
    zero, tally0 = _four_entries(E, st, ctx, seeds)
    assert all(v > 0 for v in tally0.values()), tally0
    # "a table is set" is part of the graph keys: the plain run's graphs were not replayed with the kernel missing
    assert st.counter("step_captures") > captures[0] and st.counter("beam_captures") > captures[1]
    for name in base:
        for r in range(len(base[name])):
            assert _same(base[name][r], again[name][r]), (name, r, "empty table")
            assert _same(base[name][r], zero[name][r]), (name, r, "zero boosts")
    # another table on the same buffers captures nothing again
    captures = st.counter("step_captures"), st.counter("beam_captures")
    st.set_phrase_table([top[:2], top[2:]], 0.0)
    swapped, _ = _four_entries(E, st, ctx, seeds)
    assert (st.counter("step_captures"), st.counter("beam_captures")) == captures
    assert all(_same(base[n][r], swapped[n][r]) for n in base for r in range(len(base[n])))
    # and clearing goes back to the plain run's graphs
    st.set_phrase_table(None)
    off, tally = _four_entries(E, st, ctx, seeds)
    assert set(tally.values()) == {0} and (st.counter("step_captures"), st.counter("beam_captures")) == captures
    assert all(_same(base[n][r], off[n][r]) for n in base for r in range(len(base[n])))


# ---- forced cycle ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cycle_state(E, ctx, plan):
    st = E.State(ctx, 6)
    _encode(E, st, SEEDS)
    return st


def test_forced_cycle_without_a_table_is_not_the_cycle(E, ctx, plan, cycle_state):
    """the control: the plain model does not emit the phrases by itself"""
    p = ctx.default_params(); p.n_max = N_MAX
    cycle_state.set_phrase_table(None)
    got = cycle_state.greedy_ex(2, p)
    assert got[0]["tokens"] != plan["want"][0] and got[1]["tokens"] != plan["want"][1]


@pytest.mark.parametrize("no_timestamps", [0, 1])
def test_forced_cycle_greedy(E, ctx, plans, cycle_state, no_timestamps):
    st = cycle_state
    plan = plans[no_timestamps]
    st.set_phrase_table(plan["phrases"], plan["boosts"])
    # the test entry of the kernel borrows the state's table buffers: the state's own table must be back afterwards
    other = E.phrase_table_build_host([[Q0, P[0]]], [1.0], ctx.tok.eot)
    st.dbg_phrase_boost(np.zeros((1, ctx.hp.n_vocab), np.float32), ctx.hp.n_vocab, np.zeros((1, 4), np.int32), [0], [0], other)
    p = ctx.default_params(); p.n_max = N_MAX; p.no_timestamps = no_timestamps
    got = st.greedy_ex(2, p)
    for w in range(2):
        assert got[w]["tokens"] == plan["want"][w], (w, got[w]["tokens"])
        assert not got[w]["ended_by_eot"]
        # the boost is inside the log-probabilities: a token 2 * spread above the rest has probability 1 to within MARGIN's rivals
        assert np.all(got[w]["logprobs"] > -0.2) and np.all(got[w]["logprobs"] <= 0.0)
    assert P[0] not in got[1]["tokens"]
    # the fetched row is the boosted one
    lg = st.fetch("logits", 2)
    assert lg[0].max() > plan["spread"] and lg[1].max() > plan["spread"]           # no unboosted logit is that large


def test_forced_cycle_sampler(E, ctx, plan, cycle_state):
    st = cycle_state
    st.set_phrase_table(plan["phrases"], plan["boosts"])
    p = ctx.default_params(); p.n_max = N_MAX
    got = st.sample_pass(2, T_PASS, [1, 1], _uniforms(E, 2, ctx.hp.n_text_ctx), p)
    assert [g["tokens"] for g in got] == plan["want"]


def test_forced_cycle_best_of_3(E, ctx, plan, cycle_state):
    st = cycle_state
    st.set_phrase_table(plan["phrases"], plan["boosts"])
    p = ctx.default_params(); p.n_max = N_MAX
    cap = ctx.hp.n_text_ctx
    u = _uniforms(E, 6, cap).reshape(2, 3, cap)
    assert not np.array_equal(u[0, 0], u[0, 1])
    got = st.sample_pass_n(2, 3, T_PASS, [1, 1], u, p)
    for w in range(2):
        for j in range(3):
            assert got[w * 3 + j]["tokens"] == plan["want"][w], (w, j, got[w * 3 + j]["tokens"])


def test_forced_cycle_beam_3(E, ctx, plan, cycle_state):
    st = cycle_state
    st.set_phrase_table(plan["phrases"], plan["boosts"])
    p = ctx.default_params(); p.n_max = N_MAX
    got = st.beam_search_ex(2, 3, p)
    plain = st.beam_search(2, 3, p)
    for w in range(2):
        assert got[w]["tokens"] == plan["want"][w] == plain[w]["tokens"], (w, got[w]["tokens"])
        assert got[w]["sum_logprob"] > -0.2 * N_MAX          # the boost is inside the beam scores


# ---- against a host loop -------------------------------------------------------------------------------------------------
def test_greedy_equals_a_host_loop_with_the_numpy_rule(E, ctx):
    """8 random phrases at boost 2.0 over the model's favourite tokens (a table of random ids would never match behind the root):
    ohw_greedy_ex == a loop of ohw_decode, the numpy rule and ohw_sample_greedy_host; log-probabilities within 2e-4, the bound
    test_gpu_sampler.py holds the device sampler to against the host's"""
    rng = np.random.default_rng(17)
    top = [47018, 17019, 20198, 8911, 11308]
    phrases = [[int(t) for t in rng.choice(top, size=int(rng.integers(2, 5)))] for _ in range(8)]
    table = R.build(phrases, [2.0] * 8)
    seeds = (7, 3, 11)
    B = len(seeds)
    st = E.State(ctx, B)
    _encode(E, st, seeds)
    p = ctx.default_params(); p.n_max = N_MAX
    st.set_phrase_table(phrases, 2.0)
    got = st.greedy_ex(B, p)
    st.set_phrase_table(None)
    plain = st.greedy_ex(B, p)
    assert [g["tokens"] for g in got] != [g["tokens"] for g in plain]          # the table changed the decode
    prompt = [ctx.tok.sot, ctx.tok.sot + 1 + p.lang_id, ctx.tok.transcribe]
    logits = st.decode(np.tile(np.asarray(prompt, np.int32), (B, 1)), [0] * B)
    out, lps = [[] for _ in range(B)], [[] for _ in range(B)]
    done, n_past, feed = [False] * B, [len(prompt)] * B, [0] * B
    deeper = 0
    for _ in range(N_MAX):
        for b in range(B):
            if done[b]:
                continue
            row = R.boost(table, np.asarray(out[b] + [0], np.int32), len(out[b]), logits[b])
            deeper += int(not R.same_words(row, R.boost(table, [0], 0, logits[b])))
            tok, lp = ctx.sample_greedy_host(p, row, out[b])
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
    assert deeper > 0                                                          # nodes behind the root matched along the way
    for b in range(B):
        assert got[b]["tokens"] == out[b], b
        assert np.abs(got[b]["logprobs"] - np.asarray(lps[b], np.float32)).max() < 2e-4, b


# ---- engine ----------------------------------------------------------------------------------------------------------------
def test_engine_hot_phrases_on_lanes_and_on_its_own_state(E, tmp_models):
    path = tmp_models("micro")
    pcm = np.concatenate([synth.synth_audio(40 + w) for w in range(3)])[:16000 * 70]

    def run(schedule, phrases, boost=8.0):
        eng = E.WhisperEngine.new(path, "en", False, True, 0, E.OHW_DTYPE_F16, 1)
        eng.set_decode_policy(temperature_inc=0.0)
        E.lib().ohw_engine_set_force_len(eng.h, 12)
        eng.set_schedule(schedule, lanes=2, merge=1)
        eng.set_hot_phrases(phrases, boost)
        n_set = int(E.lib().ohw_state_phrase_count(eng.state_h))
        eng.transcribe(E.AudioBuffer(pcm.copy(), 16000))
        toks = eng.last_tokens()
        eng.set_hot_phrases(None)
        assert int(E.lib().ohw_state_phrase_count(eng.state_h)) == 0
        eng.transcribe(E.AudioBuffer(pcm.copy(), 16000))
        cleared = eng.last_tokens()
        eng.close()
        return toks, cleared, n_set
    # the plain model repeats one of its favourite tokens; 8911 and 20198 lie within 2 logits of it at a window's first step, so a
    # boost of 8 on them (the root raises first tokens at every step) changes the first token of every window at least
    phrases = [[8911, 20198], [20198]]
    plain, _, n0 = run(E.OHW_SCHEDULE_SEQUENTIAL, None)
    own, own_cleared, n1 = run(E.OHW_SCHEDULE_SEQUENTIAL, phrases)
    lanes, lanes_cleared, n2 = run(E.OHW_SCHEDULE_LANES, phrases)
    assert (n0, n1, n2) == (0, 2, 2)
    assert own == lanes and own != plain and len(plain) >= 36
    assert own_cleared == plain and lanes_cleared == plain
    assert own[0] in (8911, 20198) and plain[0] not in (8911, 20198)
    # the text form: two tokenisations per text, duplicates and empty forms dropped, as the Python helper states them.  The
    # synthetic vocabulary holds " " (the blank token) and words the tokenizer's letter / digit pieces never match, so:
    # " " -> "  " = [blank, blank] and " " = [blank];  "w1" -> " w1" = [blank] again (dropped) and "w1" = nothing (dropped)
    eng = E.WhisperEngine.new(path, "en", False, True, 0, E.OHW_DTYPE_F16, 1)
    ctx = E.Context.from_file(path, 0, E.OHW_DTYPE_F16)
    blank = ctx.tok.blank
    want, boosts = E.hot_phrase_tokens(ctx, [" ", "w1"], [2.0, 3.0])
    assert (want, boosts) == ([[blank, blank], [blank]], [2.0, 2.0])
    eng.set_hot_phrases([" ", "w1"], [2.0, 3.0])
    assert int(E.lib().ohw_state_phrase_count(eng.state_h)) == 2
    with pytest.raises(E.WhisperError):
        eng.set_hot_phrases([[ctx.tok.eot]])                 # not a text token: refused, the table in effect stays
    assert int(E.lib().ohw_state_phrase_count(eng.state_h)) == 2
    eng.close()
