"""The float64 reference of one sampler call (tests/sampler_ref.py) against the oracle, and the fixtures of
test_gpu_sampler_rows.py (tests/sampler_fixtures.py) against the reference: no GPU.

1. sampler_ref.greedy agrees with oracle.Model.process_logits_ex on the committed golden rows, on every fixture row and on 300
   random rows, with and without a bias: the token, its log-probability (1e-5) and the no-speech probability.
   sampler_ref.distribution's filtered log-probabilities agree with the oracle's at the three temperatures.
2. Every fixture meets, on the reference alone, the conditions under which an fp32 kernel owes the float64 answer.  These are
   conditions, not measurements; a fixture that fails one is a bug in the fixture:
     every arg-max has gap >= 0.5 or is an exact tie by construction; every mass-rule row has ts_margin >= 0.05;
     every draw has edge >= 1e-4.
   The draw bound: the device's p_i is an fp32 expf of an fp32 difference of magnitude at most about 64, so the relative error
   of each p_i is a few 1e-6; the error of the fp32 log-sum-exp scales every p_i alike and cancels in cp / total.  1e-4 is more
   than 30 times that.  An end of a pick's interval counts only where another pick lies beyond it (sampler_ref.pick).
3. The geometry the fixtures assume."""
import ctypes as C
import os

import numpy as np
import pytest

import beam_ref as R
import sampler_fixtures as X
import sampler_ref as S
from conftest import GOLDEN
from openhush_amd import synth

GAP, MARGIN, EDGE = 0.5, 0.05, 1e-4
VOCABS = (51865, 51866)


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o
    return o


@pytest.fixture(scope="module")
def models(oracle):
    out = {}
    for V in VOCABS:
        hl = synth.PRESETS["nano"].as_list()
        hl[0] = V
        om = oracle.Model.synth(hl, 1234)
        vo = S.vocab_layout(om.n_vocab, om.tok_blank)
        assert (vo.eot, vo.sot, vo.translate, vo.transcribe, vo.solm, vo.prev, vo.nosp, vo.no_ts, vo.ts_begin, vo.n_langs) == (
            om.tok_eot, om.tok_sot, om.tok_translate, om.tok_transcribe, om.tok_solm, om.tok_prev, om.tok_nosp, om.tok_not, om.tok_beg, om.n_langs)
        assert vo.eot == S.EOT and om.n_text_ctx == 448
        out[V] = (om, vo)
    return out


def _oracle_params(om, prm, force_len=0):
    op = om.default_params()
    op.no_timestamps, op.suppress_blank, op.max_initial_ts, op.n_max, op.force_len = (prm.no_timestamps, prm.suppress_blank, prm.max_initial_ts,
                                                                                        prm.n_max, force_len)
    return op


def _check_greedy(om, vo, prm, logits, bias, hist, what, force_len=0):
    g = S.greedy(vo, prm, logits, bias, hist, force_len)
    tok, lp, ns = om.process_logits_ex(_oracle_params(om, prm, force_len), logits, hist, bias)
    assert g.token == tok, (what, g, tok)
    assert abs(g.lp - lp) < 1e-5, (what, g.lp, lp)
    assert (g.nosp is None) == (ns is None), what
    if ns is not None:
        assert abs(g.nosp - ns) < 1e-6 * max(1.0, ns) + 1e-9, (what, g.nosp, ns)
    return g


def _oracle_logprobs(oracle, om, prm, logits, bias, hist, T):
    lg = np.ascontiguousarray(logits, dtype=np.float32).copy()
    lps = np.empty_like(lg)
    c = np.asarray(hist if len(hist) else [0], dtype=np.int32)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    nul = C.cast(None, fp)
    bp = np.ascontiguousarray(bias, dtype=np.float32).ctypes.data_as(fp) if bias is not None else nul
    lp = C.c_float(0)
    oracle.lib().ref_process_logits_ex(om.h, C.byref(_oracle_params(om, prm)), lg.ctypes.data_as(fp), c.ctypes.data_as(ip), len(hist), bp, T,
                                       lps.ctypes.data_as(fp), C.byref(lp), nul)
    return lps.astype(np.float64), lg


# ------------------------------------------------------------------------------------------------ 1. the reference
def test_greedy_reference_matches_the_oracle_on_the_golden_rows(models):
    om, vo = models[51865]
    g = np.load(os.path.join(GOLDEN, "sampler.npz"))
    rows = g["rows_f16"].astype(np.float32)
    prm = R.default_params()._replace(suppress_blank=0)
    for r in range(rows.shape[0]):
        hist = [int(t) for t in g["hists"][g["hist_of_row"][r]] if t >= 0]
        got = _check_greedy(om, vo, prm, rows[r], None, hist, ("golden", r))
        assert got.token == int(g["argmax"][r]), (r, got)


@pytest.mark.parametrize("V", VOCABS)
def test_greedy_reference_matches_the_oracle_on_every_fixture_row(models, V):
    om, vo = models[V]
    prm = R.default_params()
    bias = X.F.make_bias(V)
    rows = X.greedy_rows(vo) + X.mass_rows(vo)
    for r in rows:
        v = X.effective(r, vo)
        _check_greedy(om, vo, prm, v, None, r["hist"], (V, r["name"]))
        _check_greedy(om, vo, prm, v - bias, bias, r["hist"], (V, r["name"], "bias"))
    for L in X.update_launches(vo):
        prm = R.default_params(n_max=L["n_max"])
        for r in L["rows"]:
            _check_greedy(om, vo, prm, r["v"], None, r["hist"], (V, L["name"], r["name"]), L["force_len"])


@pytest.mark.parametrize("V", VOCABS)
def test_greedy_reference_matches_the_oracle_on_random_rows(models, V):
    om, vo = models[V]
    tb = vo.ts_begin
    rng = np.random.default_rng(5 + V)
    prm = R.default_params()
    close = 0
    for k in range(150):
        row = (rng.standard_normal(V) * 3.0).astype(np.float32)
        bias = (rng.standard_normal(V) * 2.0).astype(np.float32) if k % 2 else None
        n = int(rng.integers(0, 12))
        hist = [int(t) for t in rng.integers(0, vo.eot, n)]
        for i in range(n):
            if rng.random() < 0.3:
                hist[i] = int(tb + rng.integers(0, 1500))
        if k % 5 == 0:
            row[rng.integers(0, V, 30)] = -np.inf
        g = S.greedy(vo, prm, row, bias, hist)
        if g.ts_margin < 1e-3 or g.gap < 1e-6:         # the oracle's fp32 rule may decide the other way: not a fixture, not compared
            close += 1
            continue
        _check_greedy(om, vo, prm, row, bias, hist, (V, k))
    assert close <= 8, close


@pytest.mark.parametrize("V", VOCABS)
def test_draw_reference_matches_the_oracles_filtered_probabilities(oracle, models, V):
    om, vo = models[V]
    prm = R.default_params()
    bias = X.F.make_bias(V)
    seen = set()
    for b in X.draw_batches(vo):
        kind = b["name"].rsplit("_T", 1)[0]
        if kind in ("closing_ends",):
            continue
        seen.add(kind)
        v = X.effective(b, vo)
        for use_bias in (False, True):
            lp, cp, nosp, margin, forced = S.distribution(vo, prm, v - bias if use_bias else v, bias if use_bias else None, b["hist"], b["T"])
            want, scaled = _oracle_logprobs(oracle, om, prm, v - bias if use_bias else v, bias if use_bias else None, b["hist"], b["T"])
            assert np.array_equal(lp > -np.inf, want > -np.inf), b["name"]
            ok = lp > -np.inf
            # the oracle rounds its log-sum-exp and the difference to fp32: two roundings at the magnitude of the largest value
            tol = 2.0 * float(np.spacing(np.float32(np.abs(scaled[np.isfinite(scaled)]).max()))) + 1e-6
            assert np.abs(lp[ok] - want[ok]).max() < tol, (b["name"], float(np.abs(lp[ok] - want[ok]).max()), tol)
    assert seen == {"equal_text", "ladder", "ladder_inf", "closing", "first_step", "ruler"}


# ------------------------------------------------------------------------------------------------ 2. the fixtures' conditions
@pytest.mark.parametrize("V", VOCABS)
def test_greedy_fixtures_meet_their_conditions(models, V):
    _, vo = models[V]
    prm = R.default_params()
    bias = X.F.make_bias(V)
    rows = X.greedy_rows(vo)
    names = [r["name"] for r in rows]
    assert len(set(names)) == len(names)
    by = {}
    for r in rows:
        assert np.array_equal((r["v"] - bias) + bias, r["v"]), "logits = v - bias must be exact"
        g = S.greedy(vo, prm, X.effective(r, vo), None, r["hist"])
        by[r["name"]] = g
        assert (g.gap == 0.0) if r["tie"] else (g.gap >= GAP), (r["name"], g)
        if r["name"] != "tie_ts_text":                    # exact by construction, see the fixture
            assert g.ts_margin >= MARGIN, (r["name"], g)
        if r["name"].startswith("forbidden_") or r["name"].startswith("inf_") or r["name"].startswith("hist"):
            assert r["v"][g.token] < X.F.FORBIDDEN
        if r["name"].startswith("forbidden_") or r["name"] in ("inf_hidden_winners", "inf_first_step", "hist0", "hist300_last_ts"):
            assert r["v"].max() == X.F.FORBIDDEN, r["name"]
    tb, V1 = vo.ts_begin, vo.n_vocab - 1
    want = {"win_0": 0, "win_per_m1": X.PER - 1, "win_per": X.PER, "win_7per_m1": 7 * X.PER - 1, "win_7per": 7 * X.PER,
            "win_last_live": 3 * X.PER - 1, "win_last_wave_first": X.idx(4, 448, 0), "one_thread_hi": X.idx(5, 77, 9),
            "one_thread_lo": X.idx(5, 77, 2), "win_eot_m1": vo.eot - 1, "win_eot": vo.eot, "win_ts_begin": tb, "win_last": V1,
            "win_eot_closing": vo.eot, "tie2_slices": X.idx(1, 200, 7), "tie3_slices": X.idx(0, 500, 3), "tie_one_thread": X.idx(4, 200, 2),
            "tie_ts": tb + 77, "tie_ts_text": 30000, "hist0_ts": tb + 50, "hist2_closing": tb + 5, "hist300_last_ts": tb + 400,
            "hist_longest": tb + 100, "inf_then_winner": X.idx(0, 0, 3), "inf_closing": tb}
    for name, tok in want.items():
        assert by[name].token == tok, (name, by[name], tok)
    assert not by["tie_ts_text"].forced and by["tie_ts_text"].ts_margin == 0.0 and by["tie_ts"].forced
    assert 0.01 < by["hist0"].nosp < 0.5 and 0.01 < by["inf_first_step"].nosp < 0.5
    assert len(by) >= 13 + 9 + 5 + 6 + 3


@pytest.mark.parametrize("V", VOCABS)
def test_mass_fixtures_meet_their_conditions(models, V):
    _, vo = models[V]
    prm = R.default_params()
    rows = X.mass_rows(vo)
    assert [r["name"] for r in rows] == ["mass_forced", "mass_unforced", "even_forced", "even_unforced"]
    for r in rows:
        g = S.greedy(vo, prm, r["v"], None, r["hist"])
        assert g.forced == r["forced"] and MARGIN <= g.ts_margin < 0.3, (r["name"], g)
        assert g.gap >= GAP or (r["forced"] and g.gap == 0.0), (r["name"], g)             # forced: the equal timestamps tie, the lowest is owed
        assert (g.token >= vo.ts_begin) == r["forced"]
        lp, cp, _, margin, forced = S.distribution(vo, prm, r["v"], None, r["hist"], 1.0)
        assert forced == r["forced"] and margin >= MARGIN
        targets = X.mass_targets(vo, r)
        assert len(targets) >= 3 and (min(targets) >= vo.ts_begin) == r["forced"]
        for t in targets:
            i, edge = S.pick(cp, S.midpoint(cp, t))
            assert i == t and edge >= EDGE, (r["name"], t, i, edge)
        if r["forced"]:                                   # whatever u: no text token has any probability
            assert cp[vo.ts_begin - 1] == 0.0


@pytest.mark.parametrize("V", VOCABS)
def test_draw_fixtures_meet_their_conditions(models, V):
    _, vo = models[V]
    prm = R.default_params()
    bias = X.F.make_bias(V)
    batches = X.draw_batches(vo)
    assert len({b["name"] for b in batches}) == len(batches) == 6 * len(X.TEMPS) + 1
    pos = X.ladder_positions(vo)
    for b in batches:
        assert np.array_equal((b["v"] - bias) + bias, b["v"])
        assert 2 <= len(b["want"]) <= 80
        v = X.effective(b, vo)
        lp, cp, nosp, margin, forced = S.distribution(vo, prm, v, None, b["hist"], b["T"])
        assert margin >= MARGIN, (b["name"], margin)
        us = X.with_uniforms(vo, prm, b)
        for u, t in zip(us, b["want"]):
            i, edge = S.pick(cp, u)
            assert i == t and edge >= EDGE, (b["name"], t, i, edge)
            assert b["v"][t] < X.F.FORBIDDEN and v[t] > -np.inf
        planted = np.zeros(V, bool)
        planted[b["want"]] = True
        kind = b["name"].rsplit("_T", 1)[0]
        if kind != "closing_ends":
            others = float(np.exp(lp[~planted & (lp > -np.inf)]).sum())
            assert others < 1e-3, (b["name"], others)            # the mass sits on the planted tokens
        if kind in ("equal_text", "ladder", "ladder_inf", "ruler"):
            assert not forced, b["name"]
        if kind in ("ladder", "ruler"):
            assert b["want"] == pos
        if kind == "ladder_inf":
            assert len(b["want"]) == len(pos) - 3 and 0 not in b["want"]
        if kind in ("closing", "first_step"):
            assert b["v"].max() == X.F.FORBIDDEN and (nosp is not None) == (kind == "first_step")
        if kind == "first_step":
            assert nosp > 1e-4
        if kind == "closing_ends":
            assert cp[b["want"][0] - 1] == 0.0 and cp[b["want"][1] - 1] < cp[-1] == cp[b["want"][1]]


@pytest.mark.parametrize("V", VOCABS)
def test_update_fixtures_reach_their_rules(models, V):
    _, vo = models[V]
    seen = {}
    for L in X.update_launches(vo):
        prm = R.default_params(n_max=L["n_max"])
        n_done = 0
        for r in L["rows"]:
            g = S.greedy(vo, prm, r["v"], None, r["hist"], L["force_len"])
            d = S.draw(vo, prm, r["v"], None, r["hist"], 1.0, 0.5, L["force_len"])
            assert g.gap >= GAP and g.ts_margin >= MARGIN and d.edge >= EDGE and d.token == g.token, (L["name"], r["name"], g, d)
            row = S.new_row(prm, r["hist"], r["n_past"], r["done"], r["sum_lp"])
            out, fin = S.update(prm, row, g.token, g.lp, L["advance"], L["force_len"])
            n_done += fin
            seen[L["name"] + "/" + r["name"]] = (out, fin, row)
            if r["done"]:
                assert fin == 0 and all(np.array_equal(out[k], row[k]) for k in row)
        assert n_done == sum(1 for r in L["rows"] if not r["done"] and seen[L["name"] + "/" + r["name"]][1])
    fin = {k: v[1] for k, v in seen.items()}
    assert fin["eot/eot"] and not fin["eot/plain"] and fin["n_max/at_n_max"] and not fin["n_max/short_of_n_max"]
    assert fin["force_len/reaches_force_len"] and not fin["force_len/below_force_len"] and fin["force_len/past_force_len"]
    assert fin["max_tokens/at_max_tokens"] and not fin["max_tokens/short_of_max_tokens"]
    for a in ("0", "1"):
        assert fin[f"text_ctx_advance{a}/at_ctx"] and not fin[f"text_ctx_advance{a}/short_of_ctx"] and not fin[f"text_ctx_advance{a}/plain"]
    out, _, row = seen["eot/eot"]
    assert out["next_tok"] == vo.eot and out["n_cur"] == row["n_cur"] and out["tokens"][row["n_cur"]] == S.SENT_I
    assert out["sum_logprob"] == row["sum_logprob"] and out["tok_lp"][row["n_cur"]] != float(S.SENT_F)
    out, _, row = seen["force_len/reaches_force_len"]
    assert out["next_tok"] != vo.eot and out["n_cur"] == 5
    assert seen["text_ctx_advance0/plain"][0]["n_past"] == 0 and seen["text_ctx_advance1/plain"][0]["n_past"] == 1


# ------------------------------------------------------------------------------------------------ 3. the geometry
@pytest.mark.parametrize("V", VOCABS)
def test_geometry_constants(models, V):
    _, vo = models[V]
    assert (V + 7) // 8 == X.PER == 6484 and 13 * 512 >= X.PER and 12 * 512 + 340 == X.PER
    assert ((V + 7) // 8 + 63) // 64 * 64 == X.WPER == 6528 and X.WPER % (64 * 16) == 6 * 64
    assert 7 * X.WPER + 6144 + V % 64 == V and V % 64 in (25, 26)
    assert vo.ts_begin >= 7 * X.PER and vo.ts_begin >= 7 * X.WPER
    assert V - (vo.ts_begin + 1) == 1500
