"""What ohw_beam_search_ex adds to the beam search, on the device: the per-token log-probability history that travels with the
beams (beam_update_kernel), the no-speech probability of the first step (beam_topk_kernel) and the final ranking
(beam_finish_kernel).

Row level (nano dims, the 80-row state of test_gpu_beam_step.py's rig, V = 51865 and 51866, f16 context): ohw_dbg_beam_step_ex
and ohw_dbg_beam_finish against the float64 references of tests/beam_lp_ref.py (pinned on the CPU by test_beam_finish_cpu.py).
Integers equal the reference; log-probabilities within test_gpu_beam_step.py's TOL; gathered history values are copies and
must be the input's bits; -inf and the sentinel exactly where the reference has them.

State level (micro model, three windows): ohw_beam_search_ex against ohw_beam_search (the same bits) and against the oracle's
walk along the winner."""
import numpy as np
import pytest

import beam_fixtures as F
import beam_lp_ref as L
import beam_ref as R
from openhush_amd import synth
from test_gpu_beam_step import TOL, _close, _compare, _params

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOL_LOGIT = 0.03            # f16 logits (test_gpu_policy.py's TOL): per-token log-probabilities within 2 * TOL_LOGIT


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
def rig(E):
    """per vocabulary: (context at nano dims, a state of 80 decoder rows, the vocabulary layout)"""
    out = {}
    for V in (51865, 51866):
        hl = synth.PRESETS["nano"].as_list()
        hl[0] = V
        ctx = E.Context.synthetic(hl, 1234, 0, E.OHW_DTYPE_F16)
        out[V] = (ctx, E.State(ctx, 80), R.vocab_layout(V, ctx.tok.blank))
    return out


def _with_history(state, K, prm):
    """distinct per (row, position) values, exact in fp32 and whole units apart between rows: a gather from the wrong source
    row or position is an error of at least 1e-3"""
    Rn, Ln = state["tokens"].shape[0], prm.max_tokens + 1
    i = np.arange(Ln)
    st = dict(state)
    st["plog"] = (-(np.arange(Rn)[:, None] + i[None, :] / 1024.0)).astype(np.float32).astype(np.float64)
    st["fin_plog"] = (-(500 + np.arange(Rn)[:, None] + i[None, :] / 1024.0)).astype(np.float32).astype(np.float64)
    return st


def _compare_lp(got, want, st_in, K, what):
    """plog / fin_plog: copies exactly, this step's own values within TOL, -inf and the sentinel in place"""
    _close(got["plog"], want["plog"], TOL, what + " plog")
    _close(got["fin_plog"], want["fin_plog"], TOL, what + " fin_plog")
    W = st_in["n_cur"].size
    for w in range(W):
        if st_in["win_done"][w]:
            continue
        n = int(st_in["n_cur"][w])
        rows = slice(w * K, w * K + K)
        assert np.array_equal(got["plog"][rows, :n], want["plog"][rows, :n].astype(np.float32)), (what, w, "gathered history")
        assert (got["plog"][rows, n + 1:] == L.SENT_F).all(), (what, w)
        for f in range(int(want["fin_cnt"][w])):
            m = int(want["fin_len"][w * K + f])
            assert np.array_equal(got["fin_plog"][w * K + f, :m], want["fin_plog"][w * K + f, :m].astype(np.float32)), (what, w, f, "pool history")


def _launches(vo, K):
    """test_gpu_beam_step.py's update launches (the first step, one and two sequences finishing at once with the pool at 0, K - 1
    and K entries, finished windows beside live ones, the length limits, dead beams), plus a step at n_cur = 1 and one at
    n_cur = 60 (K * n_cur > 256 at K = 5: the gather loop strides more than once)"""
    out = list(F.update_launches(vo, K))
    a, b = F._window(vo, K, 700, n_cur=1), F._window(vo, K, 701, n_cur=60)
    a["name"], b["name"] = "n_cur_1", "n_cur_60"
    # two of the long window's beams end: pool entries of 60 values are gathered too
    for j in range(2):
        b["v"][j] = F._std_row(b["base"], [vo.eot] + F.text_hist(7100 + j, K))
    out.append(dict(name="n_cur_1+n_cur_60", first=False, n_max=220, windows=[a, b]))
    return out


@pytest.mark.parametrize("K", [2, 3, 5])
@pytest.mark.parametrize("V", [51865, 51866])
def test_step_history_matches_the_reference(rig, V, K):
    ctx, st, vo = rig[V]
    st.set_logit_bias(None)
    seen = set()
    for n, Ln in enumerate(_launches(vo, K)):
        prm = R.default_params(n_max=Ln["n_max"])
        state, v = F.pack_update(vo, prm, K, Ln["windows"], Ln["first"])
        state = _with_history(state, K, prm)
        want, info = L.step_lp(vo, prm, K, Ln["first"], state, v, None)
        live = [w for w in range(2) if not state["win_done"][w]]
        assert all(info["score_gap"][w] >= 1e-2 for w in live), (Ln["name"], info["score_gap"])
        side = n & 1                                    # both halves of the double buffers
        got = st.dbg_beam_step_ex(_params(ctx, prm), K, Ln["first"], state, v, side, nosp=False)
        what = f"V={V} K={K} {Ln['name']} side={side}"
        _compare(got, want, K, what)
        _compare_lp(got, want, state, K, what)
        for w, x in enumerate(Ln["windows"]):
            seen.add(x["name"])
            new_fin = int(want["fin_cnt"][w]) - int(state["fin_cnt"][w])
            if x["name"] == "eot2_pool0":
                assert new_fin == 2                         # two sequences finish at once
            if x["name"] == f"eot1_pool{K}":
                assert new_fin == 0 and np.array_equal(got["fin_plog"][w * K:(w + 1) * K], state["fin_plog"][w * K:(w + 1) * K].astype(np.float32))
            if x["name"] == "done":
                assert (got["plog"][w * K:(w + 1) * K] == L.SENT_F).all()
            if x["name"] == "n_cur_60":
                assert new_fin == 2
            if x["name"] == "dead_beams":
                assert list(np.isneginf(got["plog"][w * K:(w + 1) * K, 3])) == [False] + [True] * (K - 1)
            if Ln["first"]:
                assert (got["plog"][w * K:(w + 1) * K, 1:] == L.SENT_F).all() and np.isfinite(got["plog"][w * K:(w + 1) * K, 0]).all()
    assert {"eot2_pool0", f"eot1_pool{K}", "done", "n_cur_1", "n_cur_60", "first_a", "dead_beams"} <= seen


@pytest.mark.parametrize("V", [51865, 51866])
def test_chained_history_matches_the_reference(rig, V):
    """test_gpu_beam_step.py's chained run (3 windows x 5 beams x 14 steps, the double buffers alternating) with the history fed
    back: after every step every beam's and every pool entry's values are the reference's"""
    ctx, st, vo = rig[V]
    st.set_logit_bias(None)
    prm = F.chain_params(vo)
    p = _params(ctx, prm)
    K, W, Ln = F.CHAIN_K, F.CHAIN_W, prm.max_tokens + 1
    zero = lambda: {"plog": np.zeros((W * K, Ln)), "fin_plog": np.zeros((W * K, Ln))}
    ref_h, dev_h = zero(), zero()
    ref_in = []

    def ref_step(first, state, lg, side):
        full = dict(state, **ref_h)
        out, _ = L.step_lp(vo, prm, K, first, full, lg, None)
        ref_in.append(full)
        ref_h["plog"], ref_h["fin_plog"] = out["plog"], out["fin_plog"]
        return out

    want = [s for _, s in F.run_chain(vo, ref_step)]

    def dev_step(first, state, lg, side):
        out = st.dbg_beam_step_ex(p, K, first, dict(state, **dev_h), lg, side, nosp=False)
        dev_h["plog"], dev_h["fin_plog"] = out["plog"], out["fin_plog"]
        return out

    for s, got in F.run_chain(vo, dev_step):
        what = f"V={V} step {s}"
        _compare(got, want[s], K, what)
        _close(got["plog"], want[s]["plog"], TOL, what + " plog")            # every value is one step's own, copied since
        _close(got["fin_plog"], want[s]["fin_plog"], TOL, what + " fin_plog")
        for w in range(W):
            if ref_in[s]["win_done"][w]:
                continue
            n = int(got["n_cur"][w])
            for j in range(K):
                r = w * K + j
                if np.isfinite(got["beam_sum"][r]):
                    assert abs(got["plog"][r, :n].astype(np.float64).sum() - got["beam_sum"][r]) < TOL * n, (what, r)
    assert list(got["win_done"]) == [1, 1, 1]


@pytest.mark.parametrize("V", [51865, 51866])
def test_null_history_is_the_plain_entry(rig, V):
    ctx, st, vo = rig[V]
    st.set_logit_bias(None)
    K = 3
    for Ln in F.update_launches(vo, K)[:3] + F.update_launches(vo, K)[-1:]:
        prm = R.default_params(n_max=Ln["n_max"])
        state, v = F.pack_update(vo, prm, K, Ln["windows"], Ln["first"])
        plain = st.dbg_beam_step(_params(ctx, prm), K, Ln["first"], state, v)
        ex = st.dbg_beam_step_ex(_params(ctx, prm), K, Ln["first"], state, v, nosp=False)
        assert set(ex) == set(plain)
        for k in plain:
            assert np.array_equal(np.asarray(ex[k]), np.asarray(plain[k])), (Ln["name"], k)
        # the history on changes nothing else either
        full = st.dbg_beam_step_ex(_params(ctx, prm), K, Ln["first"], _with_history(state, K, prm), v, nosp=bool(Ln["first"]))
        for k in plain:
            assert np.array_equal(np.asarray(full[k]), np.asarray(plain[k])), (Ln["name"], k)


@pytest.mark.parametrize("K", [2, 5])
@pytest.mark.parametrize("V", [51865, 51866])
def test_no_speech_probability_of_the_first_step(rig, V, K):
    """float64 soft-max of the biased, unfiltered row; one row where the no-speech token carries most of the mass, one where it
    carries almost none, one plain; with and without a bias.  A later step writes nothing."""
    ctx, st, vo = rig[V]
    prm = R.default_params()
    rows = np.stack([F.noise(900 + w, V) for w in range(3)])
    rows[0, vo.nosp] = 14.0                  # against 5e4 tokens of N(0, 1): most of the mass
    rows[1, vo.nosp] = -30.0
    for w in range(3):
        F.plant(rows[w], F.text_hist(950 + w, K + 1), top=12.0)
    state = R.new_state(3, K, prm)
    state["n_past_w"][:] = (2, 3, 2)
    bias = F.make_bias(V)
    for use_bias in (False, True):
        st.set_logit_bias(bias if use_bias else None)
        got = st.dbg_beam_step_ex(_params(ctx, prm), K, True, state, rows)
        plain = st.dbg_beam_step(_params(ctx, prm), K, True, state, rows)
        assert np.array_equal(got["cand_tok"], plain["cand_tok"]) and np.array_equal(got["cand_lp"], plain["cand_lp"])
        for w in range(3):
            want = L.nosp_prob(vo, rows[w], bias if use_bias else None)
            g = float(got["nosp_prob"][w])
            print(f"V={V} K={K} bias={use_bias} window {w}: no-speech probability {g:.6g}, reference {want:.6g}")
            assert abs(g - want) < 0.05 * max(want, 1e-6) + 1e-9, (w, g, want)             # the greedy loop's bound (test_gpu_sampler.py)
            assert abs(g - want) < 1e-4 * max(1.0, want) + 1e-7, (w, g, want)             # and its row-level one
        if not use_bias:
            assert got["nosp_prob"][0] > 0.5 and got["nosp_prob"][1] < 1e-12
    st.set_logit_bias(None)
    # not a first step: the sentinel stays
    Ln = F.update_launches(vo, K)[0]
    state, v = F.pack_update(vo, prm, K, Ln["windows"], False)
    got = st.dbg_beam_step_ex(_params(ctx, prm), K, False, state, v)
    assert (got["nosp_prob"] == L.SENT_F).all()


@pytest.mark.parametrize("K", [2, 3, 5])
def test_finish_kernel_matches_the_reference(E, rig, K):
    ctx, st, vo = rig[51865]
    S = ctx.hp.n_text_ctx
    for name, state, mt, tie in L.finish_cases(K, S=S):
        want, _ = L.finish(K, state, mt)
        got = st.dbg_beam_finish(K, state, mt)
        host = E.beam_finish_host(K, state, mt)
        for k in ("tokens", "n_tokens", "ended_by_eot", "n_finished"):
            assert np.array_equal(got[k], want[k]), (K, name, k, got[k], want[k])
        assert np.array_equal(got["logprobs"], want["logprobs"].astype(np.float32)), (K, name)
        assert np.array_equal(got["sum_logprob"], want["sum_logprob"].astype(np.float32)), (K, name)
        for k in got:
            assert np.array_equal(got[k], host[k]), (K, name, k)
    with pytest.raises(E.WhisperError):
        st.dbg_beam_finish(K, L.finish_cases(K, S=64)[0][1])                # rows that are not the state's token capacity
    name, state, mt, tie = L.finish_cases(K, S=S)[-1]
    with pytest.raises(E.WhisperError):
        E.State(ctx, K).dbg_beam_finish(K, state)                             # more rows than the state has


# ------------------------------------------------------------------------------------------------ state level
def _bias(om, ts_b, eot_b):
    b = np.zeros(om.n_vocab, np.float32)
    b[om.tok_beg:] = ts_b
    b[om.tok_eot] = eot_b
    return b


def test_beam_search_ex_is_beam_search_plus_what_the_policy_needs(E, oracle, tmp_models):
    path = tmp_models("micro")
    om = oracle.Model.load(path)
    ctx = E.Context.from_file(path, 0, E.OHW_DTYPE_F16)
    pcm = np.stack([synth.synth_audio(s) for s in (3, 11, 7)])
    n_max = 24
    seen_eot = seen_live = 0
    for K, bias in ((5, _bias(om, 6.0, 27.0)), (5, _bias(om, 8.0, 26.0)), (3, _bias(om, 6.0, 27.0)), (2, None)):
        st = E.State(ctx, 3 * K)
        st.set_logit_bias(bias)
        mel = st.mel(pcm, None, E.OHW_MEL_ZERO_TAIL)
        st.encode(3)
        p = ctx.default_params(); p.n_max = n_max
        plain = st.beam_search(3, K, p)
        c0 = st.counter("beam_captures")
        ex = st.beam_search_ex(3, K, p)
        assert st.counter("beam_captures") == c0 + 1            # its own pair: other pointers are baked in
        again = st.beam_search_ex(3, K, p)
        assert st.counter("beam_captures") == c0 + 1, "the second call with the same key captured again"
        assert st.beam_search(3, K, p) == plain and st.counter("beam_captures") == c0 + 1
        op = om.default_params(); op.n_max = n_max
        for w in range(3):
            g = ex[w]
            assert {k: g[k] for k in ("tokens", "sum_logprob", "n_finished")} == plain[w], (K, w)          # bit for bit
            assert again[w]["tokens"] == g["tokens"] and np.array_equal(again[w]["logprobs"], g["logprobs"])
            assert again[w]["no_speech_prob"] == g["no_speech_prob"] and again[w]["ended_by_eot"] == g["ended_by_eot"]
            n = len(g["tokens"]) + int(g["ended_by_eot"])
            assert len(g["logprobs"]) == n and n > 0
            assert abs(float(np.asarray(g["logprobs"], np.float64).sum()) - g["sum_logprob"]) < TOL * n, (K, w)
            assert g["n_finished"] > 0 or not g["ended_by_eot"]
            seen_eot += int(g["ended_by_eot"]); seen_live += int(not g["ended_by_eot"])
            s = oracle.State(om)
            s.set_encoder_output(om.encode(mel[w]))
            forced = g["tokens"] + ([om.tok_eot] if g["ended_by_eot"] else [])
            r = s.decode_pass(op, bias, 0.0, None, forced)
            assert r["tokens"] == forced and len(r["plogs"]) == len(forced)
            err = np.abs(np.asarray(g["logprobs"], np.float64) - np.asarray(r["plogs"], np.float64))
            print(f"K={K} window {w}: {len(forced)} tokens, worst |logprob - oracle| = {err.max():.4g}, no-speech {g['no_speech_prob']:.4g} / {r['no_speech_prob']:.4g}")
            assert err.max() < 2 * TOL_LOGIT, (K, w, err)
            assert abs(g["no_speech_prob"] - r["no_speech_prob"]) < 0.05 * max(r["no_speech_prob"], 1e-6) + 1e-9
    assert seen_eot and seen_live
    with pytest.raises(E.WhisperError):
        E.State(ctx, 4).beam_search_ex(1, 5)
