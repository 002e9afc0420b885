"""The sampler kernels (sampler_kernel, sampler_t_row and their update tail: openhush_amd/csrc/decode.hip) row by row against the
float64 reference of one sampler call (tests/sampler_ref.py, pinned to the oracle by test_sampler_ref_cpu.py), through
ohw_dbg_sample_ex, which returns the sampler's whole output.  No decoder runs: rows and states are crafted on the host from
the kernels' geometry (tests/sampler_fixtures.py), and test_sampler_ref_cpu.py checks on the reference alone that every
fixture keeps its decisions far enough from a tie for an fp32 implementation to owe the same answer.

Expectations: every integer output equals the reference, with no allowance for differing picks; log-probabilities and their
sums within 2e-4 (the bound of test_gpu_sampler.py and test_gpu_beam_step.py for fp32 log-probabilities); the no-speech
probability within 1e-4 * max(1, ref) + 1e-7 (test_gpu_sampler.py's); the entry's sentinel (= not written) exactly where the
reference writes nothing; the ticket words zero after every launch; a run with a logit bias (logits = v - bias) and a run
without one give identical words.

Worst errors against float64 measured on an MI355X: log-probability 3.8e-6 (the ladders at T = 0.2, values near 100), no-speech
probability 5.3e-8."""
import numpy as np
import pytest

import beam_fixtures as F
import beam_ref as R
import sampler_fixtures as X
import sampler_ref as S
from openhush_amd import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOL = 2e-4
VOCABS = (51865, 51866)
WORDS = ("tokens", "n_cur", "n_past", "done", "sum_logprob", "next_tok", "tok_lp", "nosp_prob", "tickets")


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from openhush_amd import engine
    engine.lib()
    return engine


@pytest.fixture(scope="module")
def rig(E):
    """per vocabulary: (context at nano dims, a state of 80 rows, a state of one row, the vocabulary layout)"""
    out = {}
    for V in VOCABS:
        hl = synth.PRESETS["nano"].as_list()
        hl[0] = V
        ctx = E.Context.synthetic(hl, 1234, 0, E.OHW_DTYPE_F16)
        vo = S.vocab_layout(V, ctx.tok.blank)
        t = ctx.tok
        assert (vo.eot, vo.sot, vo.translate, vo.transcribe, vo.solm, vo.prev, vo.nosp, vo.no_ts, vo.ts_begin, vo.n_langs) == (
            t.eot, t.sot, t.translate, t.transcribe, t.solm, t.prev, t.nosp, t.no_timestamps, t.timestamp_begin, t.n_langs)
        assert E.OHW_DBG_SENTINEL_I32 == S.SENT_I and E.OHW_DBG_SENTINEL_F32 == float(S.SENT_F) and vo.eot == S.EOT
        out[V] = (ctx, E.State(ctx, 80), E.State(ctx, 1), vo)
    return out


def _params(ctx, prm, force_len=0):
    p = ctx.default_params()
    p.n_max, p.no_timestamps, p.force_len = prm.n_max, prm.no_timestamps, force_len
    assert (p.suppress_blank, p.max_initial_ts, ctx.hp.n_text_ctx) == (prm.suppress_blank, prm.max_initial_ts, prm.n_text_ctx)
    return p


def _launch(st, ctx, vo, prm, rows, T=0.0, us=None, use_bias=False, advance=0, force_len=0):
    """rows: dict(v, hist, mask, [n_past, done, sum_lp]); all of one mask.  With a bias the -inf of the mask travels in it"""
    V = vo.n_vocab
    mask = rows[0].get("mask")
    assert all(r.get("mask") == mask for r in rows) and len(rows) <= st.max_batch
    if use_bias:
        std = F.make_bias(V)
        bias = std.copy()
        if mask:
            bias[X.inf_masks(vo)[mask]] = -np.inf
        lg = np.stack([r["v"] - std for r in rows])
    else:
        bias = None
        lg = np.stack([X.effective(r, vo) for r in rows])
    st.set_logit_bias(bias)
    try:
        return st.dbg_sample_ex(_params(ctx, prm, force_len), lg, [r["hist"] for r in rows], n_past=[r.get("n_past", 0) for r in rows],
                                done=[r.get("done", 0) for r in rows], advance=advance, temperature=T, uniforms=us,
                                sum_logprob=[r.get("sum_lp", 0.0) for r in rows])
    finally:
        st.set_logit_bias(None)


def _expect(vo, prm, rows, T=0.0, us=None, advance=0, force_len=0):
    """the reference's whole output of a launch -> (dict of arrays as dbg_sample_ex returns them, nosp [B] (None: not written))"""
    outs, nosp, n_done = [], [], 0
    cache = {}
    for b, r in enumerate(rows):
        st_row = S.new_row(prm, r["hist"], r.get("n_past", 0), r.get("done", 0), r.get("sum_lp", 0.0))
        if r.get("done", 0):
            outs.append(st_row)
            nosp.append(None)
            continue
        v = X.effective(r, vo)
        if T > 0:
            key = (id(r["v"]), tuple(r["hist"]))
            if key not in cache:                # a ladder batch is one row many times: filter it once
                cache[key] = S.distribution(vo, prm, v, None, r["hist"], T, force_len)
            lp, cp, ns, _, _ = cache[key]
            tok, _ = S.pick(cp, us[b])
            tok_lp = float(lp[tok])
        else:
            g = S.greedy(vo, prm, v, None, r["hist"], force_len)
            tok, tok_lp, ns = g.token, g.lp, g.nosp
        out, fin = S.update(prm, st_row, tok, tok_lp, advance, force_len)
        n_done += fin
        outs.append(out)
        nosp.append(ns)
    want = {k: np.stack([np.asarray(o[k]) for o in outs]) for k in ("tokens", "n_cur", "n_past", "done", "sum_logprob", "next_tok", "tok_lp")}
    want["n_done"] = n_done
    return want, nosp


def _compare(got, want, nosp, what, names):
    """-> (worst log-probability error, worst no-speech error)"""
    for k in ("next_tok", "tokens", "n_cur", "n_past", "done"):
        bad = np.argwhere(np.asarray(got[k]) != want[k])
        assert bad.size == 0, (what, k, [(names[int(b[0])], got[k][tuple(b)], want[k][tuple(b)]) for b in bad[:8]])
    assert got["n_done"] == want["n_done"], (what, got["n_done"], want["n_done"])
    assert not got["tickets"].any(), (what, got["tickets"])
    sent = want["tok_lp"] == float(S.SENT_F)
    assert np.array_equal(got["tok_lp"][sent], want["tok_lp"][sent].astype(np.float32)), (what, "tok_lp written where nothing is due")
    err = np.abs(got["tok_lp"].astype(np.float64) - want["tok_lp"])[~sent]
    rows_of = np.argwhere(~sent)[:, 0]
    assert np.all(np.isfinite(got["tok_lp"][~sent])) and np.all(err <= TOL), (what, "tok_lp", [(names[int(r)], float(e)) for r, e in zip(rows_of, err) if not e <= TOL][:8])
    serr = np.abs(got["sum_logprob"].astype(np.float64) - want["sum_logprob"])
    assert np.all(serr <= TOL), (what, "sum_logprob", got["sum_logprob"], want["sum_logprob"])
    worst_ns = 0.0
    for b, ns in enumerate(nosp):
        if ns is None:
            assert got["nosp_prob"][b] == np.float32(S.SENT_F), (what, names[b], "no-speech probability written for a row with a history")
        else:
            e = abs(float(got["nosp_prob"][b]) - ns)
            assert e < 1e-4 * max(1.0, ns) + 1e-7, (what, names[b], float(got["nosp_prob"][b]), ns)
            worst_ns = max(worst_ns, e)
    return (float(err.max()) if err.size else 0.0), worst_ns


def _same_words(a, b, what):
    for k in WORDS:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (what, k)
    assert a["n_done"] == b["n_done"], what


def _by_mask(rows):
    groups = {}
    for r in rows:
        groups.setdefault(r.get("mask"), []).append(r)
    return list(groups.values())


# ------------------------------------------------------------------------------------------------ the greedy kernel
@pytest.mark.parametrize("V", VOCABS)
def test_greedy_rows_match_the_reference(rig, V):
    """(a) geometry, (b) ties, (c) the mass rule, (f) histories and (h) -inf rows through sampler_kernel, with and without a bias"""
    ctx, st, _, vo = rig[V]
    prm = R.default_params()
    worst = [0.0, 0.0]
    for rows in _by_mask(X.greedy_rows(vo) + X.mass_rows(vo)):
        names = [r["name"] for r in rows]
        want, nosp = _expect(vo, prm, rows)
        plain = _launch(st, ctx, vo, prm, rows)
        biased = _launch(st, ctx, vo, prm, rows, use_bias=True)
        what = f"V={V} greedy mask={rows[0].get('mask')}"
        e = _compare(plain, want, nosp, what, names)
        _compare(biased, want, nosp, what + " bias", names)
        _same_words(plain, biased, what)
        worst = [max(worst[0], e[0]), max(worst[1], e[1])]
        for r, tok in zip(rows, plain["next_tok"]):
            if "forced" in r:
                assert (tok >= vo.ts_begin) == r["forced"], (what, r["name"], tok)
    print(f"V={V} greedy: worst |lp - reference| = {worst[0]:.3g}, worst |no-speech - reference| = {worst[1]:.3g}")


# ------------------------------------------------------------------------------------------------ the draw
@pytest.mark.parametrize("T", X.TEMPS)
@pytest.mark.parametrize("V", VOCABS)
def test_draw_batches_match_the_reference(rig, V, T):
    """(d) the ladders, (e) the ladder under a closing timestamp and at the first step, (h) under the -inf mask: row c of a batch
    draws with its own u and returns its own planted index; with and without a bias"""
    ctx, st, _, vo = rig[V]
    prm = R.default_params()
    worst = [0.0, 0.0]
    n = 0
    for b in X.draw_batches(vo):
        if b["T"] != T:
            continue
        us = X.with_uniforms(vo, prm, b)
        rows = [b] * len(us)
        names = [f"{b['name']}[{c}]->{t}" for c, t in enumerate(b["want"])]
        want, nosp = _expect(vo, prm, rows, T, us)
        assert list(want["next_tok"]) == list(b["want"])
        plain = _launch(st, ctx, vo, prm, rows, T, us)
        biased = _launch(st, ctx, vo, prm, rows, T, us, use_bias=True)
        what = f"V={V} {b['name']}"
        e = _compare(plain, want, nosp, what, names)
        _compare(biased, want, nosp, what + " bias", names)
        _same_words(plain, biased, what)
        assert list(plain["next_tok"]) == list(b["want"]), what
        worst = [max(worst[0], e[0]), max(worst[1], e[1])]
        n += 1
    assert n >= 6
    print(f"V={V} T={T}: {n} batches, worst |lp - reference| = {worst[0]:.3g}, worst |no-speech - reference| = {worst[1]:.3g}")


@pytest.mark.parametrize("V", VOCABS)
def test_mass_rule_rows_through_the_draw(rig, V):
    """(c) at T = 1: aimed draws match the reference; a forced row returns no text token whatever u"""
    ctx, st, _, vo = rig[V]
    prm = R.default_params()
    worst = 0.0
    for r in X.mass_rows(vo):
        _, cp, _, _, _ = S.distribution(vo, prm, r["v"], None, r["hist"], 1.0)
        targets = X.mass_targets(vo, r)
        us = [S.midpoint(cp, t) for t in targets]
        rows = [r] * len(us)
        want, nosp = _expect(vo, prm, rows, 1.0, us)
        assert list(want["next_tok"]) == targets
        for use_bias in (False, True):
            got = _launch(st, ctx, vo, prm, rows, 1.0, us, use_bias=use_bias)
            worst = max(worst, _compare(got, want, nosp, f"V={V} {r['name']} bias={use_bias}", [str(t) for t in targets])[0])
        if r["forced"]:
            sweep = [(c + 0.5) / 62 for c in range(62)] + [2.0 ** -30, 2.0 ** -20, 1.0 - 2.0 ** -20, 1.0 - 2.0 ** -53]
            got = _launch(st, ctx, vo, prm, [r] * len(sweep), 1.0, sweep)
            lps = got["tok_lp"][np.arange(len(sweep)), len(r["hist"])]
            assert np.all(got["next_tok"] >= vo.ts_begin) and np.all(np.isfinite(lps)), (r["name"], got["next_tok"], lps)
    print(f"V={V} mass rows at T=1: worst |lp - reference| = {worst:.3g}")


@pytest.mark.parametrize("V", VOCABS)
def test_ladder_rows_one_at_a_time_give_the_batchs_words(rig, V):
    """the ladder batch row by row on a state of ONE row: the same words as in the batch (the ticketed merge is per row)"""
    ctx, st, st1, vo = rig[V]
    prm = R.default_params()
    for b in X.draw_batches(vo):
        if not b["name"].startswith("ladder_T"):
            continue
        us = X.with_uniforms(vo, prm, b)
        batch = _launch(st, ctx, vo, prm, [b] * len(us), b["T"], us)
        for c, u in enumerate(us):
            one = _launch(st1, ctx, vo, prm, [b], b["T"], [u])
            for k in WORDS:
                assert np.asarray(one[k])[0].tobytes() == np.asarray(batch[k])[c].tobytes(), (V, b["name"], c, k)
            assert one["next_tok"][0] == b["want"][c]


# ------------------------------------------------------------------------------------------------ the update tail
@pytest.mark.parametrize("T", [0.0, 1.0])
@pytest.mark.parametrize("V", VOCABS)
def test_update_tail_matches_the_reference(rig, V, T):
    """(g) through both kernels: end-of-text, the three finishing limits, force_len, advance, a done row beside live ones"""
    ctx, st, _, vo = rig[V]
    worst = 0.0
    for L in X.update_launches(vo):
        prm = R.default_params(n_max=L["n_max"])
        rows = L["rows"]
        us = [0.5] * len(rows) if T > 0 else None
        want, nosp = _expect(vo, prm, rows, T, us, L["advance"], L["force_len"])
        got = _launch(st, ctx, vo, prm, rows, T, us, advance=L["advance"], force_len=L["force_len"])
        what = f"V={V} T={T} {L['name']}"
        worst = max(worst, _compare(got, want, nosp, what, [r["name"] for r in rows])[0])
        for b, r in enumerate(rows):
            if r["done"]:                       # nothing of a row that came in done changes
                assert got["next_tok"][b] == S.SENT_I and np.all(got["tok_lp"][b] == np.float32(S.SENT_F)) and got["done"][b] == 1
                assert got["sum_logprob"][b] == np.float32(r["sum_lp"]) and got["n_past"][b] == r["n_past"] and got["n_cur"][b] == len(r["hist"])
        assert got["n_done"] == sum(int(d) for d, r in zip(got["done"], rows) if not r["done"])
    print(f"V={V} T={T} update: worst |lp - reference| = {worst:.3g}")


@pytest.mark.parametrize("V", VOCABS)
def test_beam_first_step_under_the_inf_mask(rig, V):
    """beam_topk_kernel sums the unfiltered row for the no-speech probability as the samplers do: under the same -inf bias its
    first step owes the reference's no-speech probability and candidates"""
    ctx, st, _, vo = rig[V]
    K, prm = 2, R.default_params()
    r = next(x for x in X.greedy_rows(vo) if x["name"] == "inf_first_step")
    bias = np.zeros(V, np.float32)
    bias[X.inf_masks(vo)["first"]] = -np.inf
    state = R.new_state(1, K, prm)
    state["n_past_w"][0] = 2
    want, _ = R.step(vo, prm, K, True, state, r["v"][None], bias)
    ns = S.greedy(vo, prm, r["v"], bias, []).nosp
    st.set_logit_bias(bias)
    try:
        got = st.dbg_beam_step_ex(_params(ctx, prm), K, True, state, r["v"][None])
    finally:
        st.set_logit_bias(None)
    assert np.array_equal(got["cand_tok"], want["cand_tok"]), (got["cand_tok"], want["cand_tok"])
    err = np.abs(got["cand_lp"][0].astype(np.float64) - want["cand_lp"][0])
    assert np.all(err <= TOL), (got["cand_lp"][0], want["cand_lp"][0])
    assert abs(float(got["nosp_prob"][0]) - ns) < 1e-4 * max(1.0, ns) + 1e-7, (float(got["nosp_prob"][0]), ns)
    print(f"V={V} beam first step: |lp - reference| = {err.max():.3g}, |no-speech - reference| = {abs(float(got['nosp_prob'][0]) - ns):.3g}")


def test_entry_refuses_bad_arguments(rig, E):
    ctx, st, st1, vo = rig[51865]
    V = vo.n_vocab
    p = ctx.default_params()
    row = X.base_noise(vo)
    ok = dict(histories=[[50, 51]], n_past=[3], advance=1, temperature=1.0, uniforms=[0.5])

    def refused(state, logits, **kw):
        with pytest.raises(E.WhisperError) as ei:
            state.dbg_sample_ex(p, logits, **{**ok, **kw})
        assert ei.value.code == E.OHW_E_INVALID_ARG, ei.value

    st.dbg_sample_ex(p, row, **ok)
    refused(st1, np.stack([row, row]), histories=[[50], [51]], n_past=[0, 0], uniforms=[0.5, 0.5])      # batch > max_batch
    refused(st, row, histories=[[50] * 448])                    # n_hist == max_tokens
    refused(st, row, histories=[[50, V]])                       # a history token past the vocabulary
    refused(st, row, histories=[[-1, 50]])
    refused(st, row, n_past=[-1])
    refused(st, row, n_past=[447])                              # n_past + advance == n_text_ctx
    refused(st, row, n_past=[448], advance=0)
    refused(st, row, advance=2)
    refused(st, row, temperature=-1.0)
    refused(st, row, temperature=float("nan"))
    refused(st, row, uniforms=None)
    refused(st, row, uniforms=[1.0])
    st.dbg_sample_ex(p, row, histories=[[50] * 447], n_past=[447], advance=0, temperature=0.0)           # the limits themselves pass
    # the bias setter: -inf is a value, +inf and NaN are refused and leave the bias in effect alone
    bias = np.zeros(V, np.float32)
    bias[7] = -np.inf
    st.set_logit_bias(bias)
    for bad in (np.inf, np.nan):
        b2 = np.zeros(V, np.float32)
        b2[V - 1] = bad
        with pytest.raises(E.WhisperError) as ei:
            st.set_logit_bias(b2)
        assert ei.value.code == E.OHW_E_INVALID_ARG
    st.set_logit_bias(None)
