"""The beam step's two kernels (beam_topk_kernel, beam_update_kernel: openhush_amd/csrc/decode.hip) row by row against the
float64 host reference of one step (tests/beam_ref.py, pinned to the oracle by test_beam_ref_cpu.py), through
ohw_dbg_beam_step.  No decoder runs: rows and states are crafted on the host (tests/beam_fixtures.py), and
test_beam_ref_cpu.py checks on the reference alone that every fixture keeps its decisions far enough from a tie for an fp32
implementation to owe the same answer.

Expectations: every integer output equals the reference; log-probabilities within 2e-4 (the sampler tests' bound for fp32
log-probabilities), cumulative sums within 2e-4 per token summed; -inf and the entry's sentinel (= not written) exactly
where the reference has them; the top-k's ticket words are zero after every launch."""
import numpy as np
import pytest

import beam_fixtures as F
import beam_ref as R
from openhush_amd import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOL = 2e-4
INT_KEYS = ("tokens", "kv_slot", "n_cur", "n_past_w", "win_done", "fin_cnt", "fin_tok", "fin_len", "cand_tok", "next_tok", "n_past")


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from openhush_amd import engine
    engine.lib()
    return engine


@pytest.fixture(scope="module")
def rig(E):
    """per vocabulary: (context at nano dims, a state of 80 decoder rows, the vocabulary layout)"""
    out = {}
    for V in (51865, 51866):
        hl = synth.PRESETS["nano"].as_list()
        hl[0] = V
        ctx = E.Context.synthetic(hl, 1234, 0, E.OHW_DTYPE_F16)
        vo = R.vocab_layout(V, ctx.tok.blank)
        t = ctx.tok
        assert (vo.eot, vo.sot, vo.translate, vo.transcribe, vo.solm, vo.prev, vo.nosp, vo.no_ts, vo.ts_begin, vo.n_langs) == (
            t.eot, t.sot, t.translate, t.transcribe, t.solm, t.prev, t.nosp, t.no_timestamps, t.timestamp_begin, t.n_langs)
        assert E.OHW_DBG_SENTINEL_I32 == R.SENT_I and E.OHW_DBG_SENTINEL_F32 == float(R.SENT_F)
        out[V] = (ctx, E.State(ctx, 80), vo)
    return out


def _params(ctx, prm):
    p = ctx.default_params()
    p.n_max, p.no_timestamps = prm.n_max, prm.no_timestamps
    assert (p.suppress_blank, p.max_initial_ts, ctx.hp.n_text_ctx) == (prm.suppress_blank, prm.max_initial_ts, prm.n_text_ctx)
    return p


def _close(got, want, tol, what):
    """floats: -inf and the sentinel exactly where the reference has them, the rest within tol (scalar or per element)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    special = np.isneginf(want) | (want == float(R.SENT_F))
    assert np.array_equal(got[special], want[special]), (what, got, want)
    with np.errstate(invalid="ignore"):                 # -inf - -inf at the special places
        err = np.abs(got - want)[~special]
    lim = np.broadcast_to(tol, want.shape)[~special]
    assert np.all(np.isfinite(got[~special])) and np.all(err <= lim), (what, float(err.max()), got, want)
    return float(err.max()) if err.size else 0.0


def _compare(got, want, K, what):
    for k in INT_KEYS:
        assert np.array_equal(got[k], want[k]), (what, k, np.argwhere(np.asarray(got[k]) != np.asarray(want[k]))[:8], got[k], want[k])
    assert got["n_done"] == want["n_done"], (what, got["n_done"], want["n_done"])
    assert not got["tickets"].any(), (what, got["tickets"])
    worst = _close(got["cand_lp"], want["cand_lp"], TOL, what + " cand_lp")
    n_sum = np.repeat(np.maximum(1, want["n_cur"]), K)                         # tokens summed into a beam's score
    _close(got["beam_sum"], want["beam_sum"], TOL * n_sum, what + " beam_sum")
    _close(got["fin_sum"], want["fin_sum"], TOL * (np.maximum(0, want["fin_len"]) + 1), what + " fin_sum")       # + end-of-text's
    return worst


# ------------------------------------------------------------------------------------------------ (a) top-k geometry
@pytest.mark.parametrize("K", [2, 3, 5])
@pytest.mark.parametrize("V", [51865, 51866])
def test_topk_candidates_match_the_reference(rig, V, K):
    """One row per geometry, tie, forbidden-token, history, few-allowed and timestamp-mass case (beam_fixtures.topk_rows), packed
    into windows by history length; with and without a logit bias (the same effective rows), with and without no_timestamps."""
    ctx, st, vo = rig[V]
    rows = F.topk_rows(vo, K)
    bias = F.make_bias(V)
    worst = (0.0, None)
    for no_ts in (0, 1):
        prm = R.default_params(no_timestamps=no_ts)
        state, v, names = F.pack_topk(vo, prm, K, rows)
        want, info = R.step(vo, prm, K, False, state, v, None)
        for use_bias in (False, True):
            st.set_logit_bias(bias if use_bias else None)
            got = st.dbg_beam_step(_params(ctx, prm), K, False, state, v - bias if use_bias else v)
            what = f"V={V} K={K} no_ts={no_ts} bias={use_bias}"
            bad = np.argwhere(got["cand_tok"] != want["cand_tok"])
            assert bad.size == 0, (what, [(names[r], list(got["cand_tok"][r]), list(want["cand_tok"][r])) for r in sorted({int(b[0]) for b in bad})])
            with np.errstate(invalid="ignore"):
                err = np.abs(got["cand_lp"].astype(np.float64) - want["cand_lp"])
            err[~np.isfinite(want["cand_lp"])] = 0
            r = int(err.max(axis=1).argmax())
            if err.max() > worst[0]:
                worst = (float(err.max()), what + " row " + names[r])
            print(f"{what}: worst |cand_lp - reference| = {err.max():.3g} (row {names[r]})")
            _close(got["cand_lp"], want["cand_lp"], TOL, what)
            assert not got["tickets"].any()
            if not no_ts:
                # a row with fewer than K + 1 allowed tokens: the tails say so
                r = names.index("few_forced")
                assert list(got["cand_tok"][r, 2:]) == [-1] * (K - 1) and np.all(np.isneginf(got["cand_lp"][r, 2:])), what
    st.set_logit_bias(None)
    print(f"worst of all: {worst}")


# ------------------------------------------------------------------------------------------------ (b) update rules
@pytest.mark.parametrize("K", [2, 3, 5])
@pytest.mark.parametrize("V", [51865, 51866])
def test_update_rules_match_the_reference(rig, V, K):
    """Two windows with different states per launch (beam_fixtures.update_launches): sources, end-of-text and the pool, ties,
    finished windows, the three length limits, the first step, and the dead-beam state."""
    ctx, st, vo = rig[V]
    st.set_logit_bias(None)
    seen_dead = False
    for L in F.update_launches(vo, K):
        prm = R.default_params(n_max=L["n_max"])
        state, v = F.pack_update(vo, prm, K, L["windows"], L["first"])
        want, info = R.step(vo, prm, K, L["first"], state, v, None)
        got = st.dbg_beam_step(_params(ctx, prm), K, L["first"], state, v)
        what = f"V={V} K={K} {L['name']}"
        for w, x in enumerate(L["windows"]):
            if x["name"] == "dead_beams":
                # the oracle's rule, stated on the device's own output: a dead beam proposes nothing
                seen_dead = True
                print(f"{what}: device fin_cnt {got['fin_cnt'][w]}, fin_sum {got['fin_sum'][w * K:w * K + K]}, beam_sum "
                      f"{got['beam_sum'][w * K:w * K + K]}, win_done {got['win_done'][w]}")
                assert got["fin_cnt"][w] == 1 and np.isfinite(got["fin_sum"][w * K]) and got["win_done"][w] == 0, what
                assert not np.isneginf(got["fin_sum"][w * K:w * K + K]).any(), what
                assert list(np.isfinite(got["beam_sum"][w * K:w * K + K])) == [True] + [False] * (K - 1), what
        _compare(got, want, K, what)
        if "n_done" in L:
            assert got["n_done"] == L["n_done"] and list(got["win_done"]) == L["done_after"], what
    assert seen_dead


# ------------------------------------------------------------------------------------------------ (c) a chained run
_ref_chain = {}


def _reference_chain(vo):
    if vo.n_vocab not in _ref_chain:
        prm = F.chain_params(vo)
        _ref_chain[vo.n_vocab] = [st for _, st in F.run_chain(vo, lambda first, st, lg, side: R.step(vo, prm, F.CHAIN_K, first, st, lg, None)[0])]
    return _ref_chain[vo.n_vocab]


@pytest.mark.parametrize("V", [51865, 51866])
def test_chained_steps_match_the_reference(rig, V):
    """3 windows x 5 beams x 14 steps, the device's own state fed back through the entry with the double buffers alternating; the
    logits are a fixed function of (window, token history).  Compared with the chained reference after every step."""
    ctx, st, vo = rig[V]
    st.set_logit_bias(None)
    prm = F.chain_params(vo)
    p = _params(ctx, prm)
    want = _reference_chain(vo)
    for s, got in F.run_chain(vo, lambda first, state, lg, side: st.dbg_beam_step(p, F.CHAIN_K, first, state, lg, side)):
        _compare(got, want[s], F.CHAIN_K, f"V={V} step {s}")
    assert list(got["win_done"]) == [1, 1, 1]


# ------------------------------------------------------------------------------------------------ the entry itself
def test_entry_checks_its_arguments_and_leaves_beam_search_alone(E, rig):
    ctx, st, vo = rig[51865]
    K = 3
    prm = R.default_params()
    p = _params(ctx, prm)
    L = F.update_launches(vo, K)[0]
    state, v = F.pack_update(vo, prm, K, L["windows"], False)

    def bad(key, idx, value, K_=K):
        s2 = {k: np.array(a, copy=True) for k, a in state.items()}
        if key:
            s2[key][idx] = value
        with pytest.raises(E.WhisperError):
            st.dbg_beam_step(p, K_, False, s2, v)

    bad("n_cur", 0, prm.max_tokens)
    bad("n_cur", 1, -1)
    bad("n_past_w", 0, prm.n_text_ctx - 1)
    bad("kv_slot", (1, 2), 2 * K)
    bad("kv_slot", (0, 0), -1)
    bad("fin_cnt", 1, K + 1)
    bad("tokens", (K, 1), vo.n_vocab)
    with pytest.raises(E.WhisperError):
        st.dbg_beam_step(p, K, False, state, v, side=2)
    with pytest.raises(E.WhisperError):
        E.State(ctx, 2 * K - 1).dbg_beam_step(p, K, False, state, v)            # rows > max_batch
    for K_ in (1, 6):
        s2 = R.new_state(2, K_, prm)
        with pytest.raises(E.WhisperError):
            st.dbg_beam_step(p, K_, False, s2, np.zeros((2 * K_, vo.n_vocab), np.float32))
    # a beam search on a state the entry ran on gives what it gives on a fresh state
    pcm = np.stack([synth.synth_audio(s) for s in (3, 11)])
    q = ctx.default_params(); q.n_max = 10
    res = []
    for used in (False, True):
        s1 = E.State(ctx, 2 * K)
        if used:
            s1.dbg_beam_step(p, K, False, state, v)
        s1.mel(pcm, None, E.OHW_MEL_ZERO_TAIL, want=False)
        s1.encode(2)
        res.append(s1.beam_search(2, K, q))
        if used:
            s1.dbg_beam_step(p, K, False, state, v, side=1)
            assert s1.beam_search(2, K, q) == res[-1]
    assert res[0] == res[1]
