"""Command lists through the decoders (ohw_state_set_command_table): the rule inside ohw_greedy_ex, ohw_sample_pass,
ohw_sample_pass_n and ohw_beam_search_ex.  Micro model (f16), 3 windows, n_max 32.

Off means off: no list, and a list set and cleared again, give the bits of the plain run in all four decoders, launch nothing and
capture nothing.
Against a host loop (fails without the feature): ohw_greedy_ex under a list at p = 3 equals ohw_decode + the numpy rule +
ohw_sample_greedy_host step by step, alone and behind a hot-phrase table and the repetition rule; with the three in another order
the same comparison must fail.  The loop also yields the float64 list_logprob of each window's latest step without a text token,
which ohw_state_command_list_logprob must match within command_ref.lp_tol.
Invariant: under p = +inf the text tokens of every row every decoder returns are exactly one listed phrase.
Graphs: swapping lists and penalties captures nothing.
"""
import math

import numpy as np
import pytest

import command_ref as C
import phrase_ref as P
import repeat_ref as R
from openhush_amd import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N_MAX = 32
SEEDS = (7, 3, 11)
T_PASS = 0.4
DECODERS = ("greedy", "sample", "sample_n", "beam")
TOP = [47018, 17019, 20198, 8911, 11308]            # tokens the procedural model favours
LIST = [[47018, 17019], [47018, 17019, 20198], [8911], [11308, 8911, 47018, 17019, 20198, 8911], [17019, 17019, 17019], [20198, 11308],
        [47018, 17019]]
LIST2 = [[11308], [8911, 8911], [20198, 47018, 47018]]


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


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _same(a, b):
    return (a["tokens"] == b["tokens"] and a["ended_by_eot"] == b["ended_by_eot"] and np.array_equal(_bits(a["logprobs"]), _bits(b["logprobs"]))
            and _bits(a["no_speech_prob"]) == _bits(b["no_speech_prob"]))


def _four_entries(E, st, ctx, K=3):
    """the four decoders on the same windows -> their results, and the command_rule tally each of them added"""
    cap = ctx.hp.n_text_ctx
    W = len(SEEDS)
    p = _params(ctx)
    out, tally = {}, {}
    c0 = st.counter("command_rule")

    def took(name):
        nonlocal c0
        c1 = st.counter("command_rule")
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


def _text(tokens, eot):
    return [t for t in tokens if t < eot]


# ---- off means off -------------------------------------------------------------------------------------------------------
def test_off_means_off(E, ctx):
    st = E.State(ctx, 9)
    st.set_logit_bias(_bias(ctx))
    assert st.command_count() == 0
    base, tally = _four_entries(E, st, ctx)
    assert set(tally.values()) == {0}
    captures = _captures(st)
    st.set_command_table(None)
    st.set_command_table([], 50.0)
    again, tally = _four_entries(E, st, ctx)
    assert set(tally.values()) == {0} and _captures(st) == captures and st.command_count() == 0
    for name in DECODERS:
        assert len(base[name]) == len(again[name])
        assert all(_same(base[name][r], again[name][r]) for r in range(len(base[name]))), name
    with pytest.raises(E.WhisperError):
        st.command_list_logprob(3)                                       # no list, no list probability
    # on, then off again: the plain run's graphs serve, its bits come back
    st.set_command_table(LIST, 100.0)
    assert st.command_count() == len(LIST)
    on, tally_on = _four_entries(E, st, ctx)
    assert all(v > 0 for v in tally_on.values()), tally_on
    assert _captures(st)[0] > captures[0] and _captures(st)[1] > captures[1]        # "a list is set" is part of the graph keys
    assert any(not _same(base["greedy"][r], on["greedy"][r]) for r in range(len(SEEDS)))
    captures = _captures(st)
    st.set_command_table(None)
    off, tally = _four_entries(E, st, ctx)
    assert set(tally.values()) == {0} and _captures(st) == captures
    assert all(_same(base[n][r], off[n][r]) for n in DECODERS for r in range(len(base[n])))
    for bad in (0.0, -1.0, float("nan"), 1001.0):
        with pytest.raises(E.WhisperError) as ex:
            st.set_command_table(LIST, bad)
        assert ex.value.code == E.OHW_E_INVALID_ARG
    with pytest.raises(E.WhisperError):
        st.set_command_table([[ctx.tok.eot]], 10.0)
    assert st.command_count() == 0


# ---- against a host loop -------------------------------------------------------------------------------------------------
def _host_loop(ctx, st, p, B, modify):
    """ohw_decode + modify(row, history) -> (row, list_logprob or None) + ohw_sample_greedy_host, step by step, on the device's own
    logits -> (tokens, logprobs, the latest list_logprob per window)"""
    prompt = [ctx.tok.sot, ctx.tok.sot + 1 + p.lang_id, ctx.tok.transcribe]
    logits = st.decode(np.tile(np.asarray(prompt, np.int32), (B, 1)), [0] * B)
    out, lps, llp = [[] for _ in range(B)], [[] for _ in range(B)], [None] * B
    done, n_past, feed = [False] * B, [len(prompt)] * B, [0] * B
    for _ in range(N_MAX):
        for b in range(B):
            if done[b]:
                continue
            row, lp = modify(logits[b], out[b])
            if lp is not None:
                llp[b] = lp
            tok, tlp = ctx.sample_greedy_host(p, row, out[b])
            lps[b].append(tlp)
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
    return out, lps, llp


@pytest.mark.parametrize("with_others", [False, True], ids=["list_alone", "behind_boost_and_repetition"])
def test_greedy_equals_a_host_loop_with_the_numpy_rule(E, ctx, with_others):
    """tokens exactly (the loop works on the device's own logits), log-probabilities within 2e-4, the bound test_gpu_sampler.py
    holds the device sampler to against the host's; list_logprob within command_ref.lp_tol of the loop's float64 value.
    Alone the list runs at p = 100.  Behind the boost and the repetition rule (2.0, 3) it runs at p = 1.5, 4, 10 and 25: the order
    of the three shows only where a token of the history that is not a child keeps some probability (x / theta - p against
    (x - p) / theta), which depends on how p compares with the model's margins; the right order must agree at every p, each wrong
    order must fail the same comparison at one of them at least"""
    theta, n = 2.0, 3
    eot = ctx.tok.eot
    B = len(SEEDS)
    rng = np.random.default_rng(17)
    phrases = [[int(t) for t in rng.choice(TOP, size=int(rng.integers(2, 5)))] for _ in range(8)]
    table = P.build(phrases, [2.0] * 8)
    st = E.State(ctx, B)
    _encode(E, st)
    p = _params(ctx)
    plain = st.greedy_ex(B, p)

    def hist(h):
        return np.asarray(h + [0], np.int32)

    def boost(row, h):
        return P.boost(table, hist(h), len(h), row) if with_others else row

    def repeat(row, h):
        return R.rule(theta, n, hist(h), len(h), row, eot) if with_others else row
    disagree = {"list_first": [], "list_second": []}
    for pen in ((1.5, 4.0, 10.0, 25.0) if with_others else (100.0,)):
        st.set_command_table(LIST, pen)
        if with_others:
            st.set_phrase_table(phrases, 2.0)
            st.set_repeat_rule(theta, n)
        got = st.greedy_ex(B, p)
        dev_lp = st.command_list_logprob(B)
        assert st.counter("command_rule") > 0
        assert [g["tokens"] for g in got] != [g["tokens"] for g in plain]              # the rules changed the decode
        st.set_command_table(None)
        st.set_repeat_rule()
        st.set_phrase_table(None)
        l_max = [0.0]                                                    # the largest |logit| of a row whose list_logprob was taken

        def right(row, h):
            row = repeat(boost(row, h), h)
            if not _text(h, eot):
                l_max[0] = max(l_max[0], float(np.abs(row[:eot][np.isfinite(row[:eot])]).max()))
            return C.rule(LIST, pen, hist(h), len(h), row, eot)

        def list_first(row, h):
            row, lp = C.rule(LIST, pen, hist(h), len(h), row, eot)
            return repeat(boost(row, h), h), lp

        def list_second(row, h):
            row, lp = C.rule(LIST, pen, hist(h), len(h), boost(row, h), eot)
            return repeat(row, h), lp

        def far(loop):
            """per window: the tokens differ, or else the largest log-probability difference"""
            out, lps, _ = loop
            return [math.inf if got[b]["tokens"] != out[b] or len(lps[b]) != len(got[b]["logprobs"])
                    else float(np.abs(got[b]["logprobs"] - np.asarray(lps[b], np.float32)).max()) for b in range(B)]
        loop = _host_loop(ctx, st, p, B, right)
        tol = C.lp_tol(eot, l_max[0])                                    # command_ref's bound at these rows' own magnitude
        print("p", pen, "right order", far(loop), "list_logprob", dev_lp.tolist(), "float64", loop[2], "tolerance", tol, "largest |logit|", l_max[0])
        for b in range(B):
            assert got[b]["tokens"] == loop[0][b], (pen, b)
        assert max(far(loop)) < 2e-4, pen
        assert all(lp is not None and math.isfinite(lp) for lp in loop[2])
        assert np.abs(dev_lp.astype(np.float64) - np.asarray(loop[2])).max() <= tol, pen
        if with_others:
            for name, fn in (("list_first", list_first), ("list_second", list_second)):
                f = far(_host_loop(ctx, st, p, B, fn))
                print("p", pen, name, f)
                disagree[name].append(max(f) >= 2e-4)
    if with_others:
        assert any(disagree["list_first"]) and any(disagree["list_second"]), disagree


# ---- the invariant -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("biased", [False, True], ids=["plain_rows", "timestamps_and_eot_compete"])
def test_hard_list_every_row_of_every_decoder_is_one_listed_phrase(E, ctx, biased):
    """p = +inf, n_max 32 above the longest phrase (6 tokens, and a pair of timestamps between any two): by construction, for any
    draw - greedy, the temperature pass at T = 0.4, 3 candidates per window, 5 beams"""
    eot = ctx.tok.eot
    st = E.State(ctx, 15)
    if biased:
        st.set_logit_bias(_bias(ctx))
    st.set_command_table(LIST, math.inf)
    out, tally = _four_entries(E, st, ctx, K=5)
    assert all(v > 0 for v in tally.values()), tally
    assert len(out["sample_n"]) == 3 * len(SEEDS) and len(out["beam"]) == len(SEEDS)
    table = E.command_table_build_host(LIST, eot)
    n_rows = 0
    for name in DECODERS:
        for r, g in enumerate(out[name]):
            assert _text(g["tokens"], eot) in LIST, (name, r, g["tokens"])
            assert g["ended_by_eot"], (name, r, g["tokens"])
            assert E.command_match_host(table, g["tokens"]) == LIST.index(_text(g["tokens"], eot))
            n_rows += 1
    assert n_rows == 3 + 3 + 9 + 3
    lp = st.command_list_logprob(len(SEEDS))
    assert np.all(np.isfinite(lp)) and np.all(lp < 0)


# ---- graphs ----------------------------------------------------------------------------------------------------------------
def test_swapping_lists_and_penalties_captures_nothing(E, ctx):
    st = E.State(ctx, 1)
    _encode(E, st, SEEDS[:1])
    p = _params(ctx)
    eot = ctx.tok.eot
    run = lambda: st.greedy_ex(1, p)[0]["tokens"]
    plain = run()
    c_plain = _captures(st)
    st.set_command_table(LIST, math.inf)
    a = run()
    c_on = _captures(st)
    assert c_on[0] == c_plain[0] + 1 and _text(a, eot) in LIST
    st.set_command_table(LIST2, math.inf)                  # another list in the same buffer: the captured step serves
    b = run()
    assert _captures(st) == c_on and _text(b, eot) in LIST2
    st.set_command_table(LIST2, 0.001)                     # a penalty too small to matter
    c = run()
    assert _captures(st) == c_on and _text(c, eot) == _text(plain, eot)
    st.set_command_table(None)
    assert run() == plain and _captures(st) == c_on
    st.set_command_table(LIST, math.inf)
    assert run() == a and _captures(st) == c_on
