"""The host reference of one beam step (tests/beam_ref.py) against the oracle, and the fixtures of test_gpu_beam_step.py
(tests/beam_fixtures.py) against the reference: no GPU.

1. Chained reference steps, fed with the oracle decoder's logits on the nano model, reproduce oracle.beam_search: the winner,
   n_finished and every final candidate.  The filter is pinned row by row to ref_process_logits' log-probabilities.
2. Every crafted fixture meets the gap conditions under which an fp32 implementation must agree exactly with float64:
   (a) planted values 1.0 apart and 8 above the noise, the timestamp-mass comparison at least 0.1 nat from its threshold;
   (b) every gap between ranked cumulative scores exactly 0 or at least 1e-2;
   (c) the chained run: every gap the update loop's outcome depends on is 0 or at least 1e-3; its windows finish through three
       different rules and one of them passes a step with fewer than K live beams.
       1e-3 from the number formats: a candidate's fp32 log-probability is v - (M + log S) with |v|, |M| < 64 (ulp 4e-6) and S
       summed from about 50 partial sums per token path (26 per lane, 6 + 2 shuffle and wave stages, 8 slices; relative error
       below 50 x 2^-24 = 3e-6 on log S's argument, plus expf / logf at a few ulp): below 1e-5 per candidate.  A cumulative
       score adds at most 14 of them in fp32 at magnitudes below 64 (ulp 4e-6 per addition): below 14 x 1.4e-5 = 2e-4 per
       score, 4e-4 between two scores; 1e-3 leaves a factor 2.5."""
import numpy as np
import pytest

import beam_fixtures as F
import beam_ref as R
from openhush_amd import synth


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o
    return o


def _nano(oracle, V=51865):
    hl = synth.PRESETS["nano"].as_list()
    hl[0] = V
    return oracle.Model.synth(hl, 1234)


def _vocab(om):
    vo = R.vocab_layout(om.n_vocab, om.tok_blank)
    assert (vo.eot, vo.sot, vo.translate, vo.transcribe, vo.solm, vo.prev, vo.nosp, vo.no_ts, vo.ts_begin, vo.n_langs) == (
        om.tok_eot, om.tok_sot, om.tok_translate, om.tok_transcribe, om.tok_solm, om.tok_prev, om.tok_nosp, om.tok_not, om.tok_beg, om.n_langs)
    return vo


@pytest.fixture(scope="module")
def vocabs(oracle):
    return {V: _vocab(_nano(oracle, V)) for V in (51865, 51866)}


def _bias(om, ts_b, eot_b):
    b = np.zeros(om.n_vocab, np.float32)
    b[om.tok_beg:] = ts_b
    b[om.tok_eot] = eot_b
    return b


@pytest.fixture(scope="module")
def nano_enc(oracle):
    om = _nano(oracle)
    return om, om.encode(om.log_mel(synth.synth_audio(3), 0))


@pytest.mark.parametrize("no_ts", [0, 1])
@pytest.mark.parametrize("K", [2, 3, 5])
def test_chained_reference_steps_reproduce_the_oracle_beam_search(oracle, nano_enc, K, no_ts):
    om, enc = nano_enc
    vo = _vocab(om)
    n_max = 16
    pinned = 0
    # test_gpu_beam.py's two biases end the nano model's windows at once; the others run 4 to 16 steps, with pools that fill at
    # different steps, pools that stay partly empty, and timestamps
    for bias in (_bias(om, 6.0, 27.0), _bias(om, 8.0, 26.0), _bias(om, 6.0, 22.0), _bias(om, 8.0, 19.0), _bias(om, 10.0, 20.0)):
        op = om.default_params(); op.n_max = n_max; op.no_timestamps = no_ts
        want = oracle.beam_search(om, enc, op, K, bias)
        prompt = om.build_prompt(op)
        prm = R.default_params(n_max=min(n_max, om.n_text_ctx - len(prompt)), no_timestamps=no_ts, n_text_ctx=om.n_text_ctx)
        st = R.new_state(1, K, prm)
        st["n_past_w"][0] = len(prompt) - 1
        dec = oracle.State(om)
        dec.set_encoder_output(enc)
        first = True
        while not st["win_done"][0]:
            n_cur = int(st["n_cur"][0])
            hists = [[int(t) for t in st["tokens"][j, :n_cur]] for j in range(1 if first else K)]
            # a beam's logits: the decoder on its whole sequence (dead beams are duplicates: any row will do)
            logits = np.stack([dec.decode(prompt + h, 0) for h in hists])
            if pinned < 40:                       # the filter, row by row, against the oracle's log-probabilities
                for h, row in zip(hists, logits):
                    lp, _, _ = R.filter_row(vo, prm, row, bias, h)
                    _, _, _, want_lp = om.process_logits(op, row + bias, h)
                    assert np.array_equal(lp > -np.inf, want_lp > -np.inf)
                    ok = lp > -np.inf
                    assert np.abs(lp[ok] - want_lp[ok]).max() < 1e-5
                    pinned += 1
            st, _ = R.step(vo, prm, K, first, st, logits, bias)
            first = False
        cands, best = R.final_candidates(K, st, 0)
        assert cands[best][0] == want["tokens"], (K, no_ts, cands[best], want)
        assert int(st["fin_cnt"][0]) == want["n_finished"]
        assert [c[0] for c in cands] == [c[0] for c in want["candidates"]]
        assert np.abs(np.array([c[1] for c in cands]) - np.array([c[1] for c in want["candidates"]])).max() < 1e-4
        assert abs(cands[best][1] - want["sum_logprob"]) < 1e-4


# ------------------------------------------------------------------------------------------------ the GPU fixtures
@pytest.mark.parametrize("V", [51865, 51866])
@pytest.mark.parametrize("K", [2, 3, 5])
def test_topk_fixtures_meet_their_gap_conditions(vocabs, V, K):
    vo = vocabs[V]
    rows = F.topk_rows(vo, K)
    bias = F.make_bias(V)
    names = [r["name"] for r in rows]
    assert len(set(names)) == len(names)
    for no_ts in (0, 1):
        prm = R.default_params(no_timestamps=no_ts)
        for r in rows:
            assert np.array_equal((r["v"] - bias) + bias, r["v"]), "logits = v - bias must be exact"
            lp, margin, forced = R.filter_row(vo, prm, r["v"], None, r["hist"])
            tok, clp, gap = R.top_candidates(lp, K)
            assert margin >= 0.1, (r["name"], margin)
            if no_ts:
                continue
            if r["spaced"]:
                assert gap >= 1.0 - 1e-9 and (tok >= 0).all(), (r["name"], gap)
                assert r["v"][tok].min() >= 11.0 and F.noise(0, V).max() <= 3.0          # planted: 8 above the noise
            if r["name"].startswith("forbidden_") or r["name"].startswith("initial_"):
                assert r["v"].max() == F.FORBIDDEN and r["v"][tok].max() < F.FORBIDDEN
            if r["name"] == "few_forced":
                assert forced and list(tok[2:]) == [-1] * (K - 1) and np.all(clp[2:] == -np.inf)
            if r["name"] == "few_unforced":
                assert not forced and list(tok[3:]) == [-1] * (K - 2)
            if r["name"] == "mass_forced":
                assert forced and margin < 0.3 and list(tok) == [vo.ts_begin + 100 + c for c in range(K + 1)]
            if r["name"] == "mass_unforced":
                assert not forced and margin < 0.3 and tok.max() < vo.eot
            if r["name"] == "tie_ts_text":
                assert not forced and list(tok[K - 1:]) == [30000, vo.ts_begin + 30] and clp[K - 1] == clp[K]
            if r["name"] == "tie_one_lane_cut":
                per = (V + 7) // 8
                assert list(tok) == [per + 99 + 256 * (2 + 3 * c) for c in range(K + 1)] and len(set(clp)) == 1
            if r["name"] == "one_lane":
                per = (V + 7) // 8
                assert {(int(t) - 2 * per) % 256 for t in tok} == {37} and {int(t) // per for t in tok} == {2}


@pytest.mark.parametrize("V", [51865, 51866])
@pytest.mark.parametrize("K", [2, 3, 5])
def test_update_fixtures_meet_their_gap_conditions(vocabs, V, K):
    vo = vocabs[V]
    seen = set()
    for L in F.update_launches(vo, K):
        prm = R.default_params(n_max=L["n_max"])
        st, v = F.pack_update(vo, prm, K, L["windows"], L["first"])
        out, info = R.step(vo, prm, K, L["first"], st, v, None)
        live = [w for w in range(2) if not st["win_done"][w]]
        assert all(info["score_gap"][w] >= 1e-2 for w in live), (L["name"], info["score_gap"])
        assert all(m >= 0.1 for m in info["ts_margin"]), (L["name"], info["ts_margin"])
        if "n_done" in L:
            assert out["n_done"] == L["n_done"] and list(out["win_done"]) == L["done_after"], L["name"]
        for w, x in enumerate(L["windows"]):
            seen.add(x["name"])
            rows = slice(w * K, w * K + K)
            if x["name"] == "one_source":
                assert info["saved"][w] == K and len({tuple(t) for t in out["tokens"][rows, :3]}) == 1
            if x["name"] == "permutation":
                assert [list(out["tokens"][w * K + i, :3]) for i in range(K)] == [x["hists"][j] for j in x["perm"]]
            if x["name"].startswith("eot"):
                n_eot, fin = (int(x["name"][3]), int(x["name"].split("pool")[1])) if "pool" in x["name"] else (0, 0)
                assert out["fin_cnt"][w] == min(K, fin + n_eot), x["name"]
                assert out["win_done"][w] == int(min(K, fin + n_eot) >= K)
            if x["name"] == "eot_below_cut":
                assert out["fin_cnt"][w] == 0 and info["saved"][w] == K
            if x["name"] in ("tie_inside", "tie_at_cut"):
                assert info["score_gap"][w] >= 1e-2 and info["saved"][w] == K
            if x["name"] == "dead_beams":
                # the oracle's rule: the live beam's end-of-text goes to the pool, its timestamp is the one continuation
                assert info["saved"][w] == 1 and out["fin_cnt"][w] == 1 and np.isfinite(out["fin_sum"][w * K])
                assert list(out["beam_sum"][rows] > -np.inf) == [True] + [False] * (K - 1) and out["win_done"][w] == 0
    assert {"one_source", "permutation", "eot1_pool0", f"eot2_pool{K}", "eot_below_cut", "tie_inside", "dead_beams", "done", "n_max",
            "max_tokens", "text_ctx", "first_a"} <= seen


@pytest.mark.parametrize("V", [51865, 51866])
def test_chain_fixture_meets_its_conditions(vocabs, V):
    vo = vocabs[V]
    prm = F.chain_params(vo)
    K = F.CHAIN_K
    infos, done_at = [], {}

    def ref_step(first, st, logits, side):
        out, info = R.step(vo, prm, K, first, st, logits, None)
        infos.append((info, st["win_done"].copy(), out))
        return out

    for s, st in F.run_chain(vo, ref_step):
        for w in range(F.CHAIN_W):
            if st["win_done"][w] and w not in done_at:
                done_at[w] = s
    few_live = False
    for info, was_done, out in infos:
        for w in range(F.CHAIN_W):
            if was_done[w]:
                continue
            assert info["decided_gap"][w] >= 1e-3, (w, info["decided_gap"])
            few_live |= 0 < info["n_live_in"][w] < K
        assert all(m >= 0.1 for m in info["ts_margin"])
    assert few_live, "no window passed a step with fewer than K live beams"
    last = infos[-1][2]
    # window 0: its pool is full; window 1: n_max; window 2: the text context - three different rules, at different steps
    assert last["fin_cnt"][0] == K and done_at[0] < F.CHAIN_STEPS - 1
    assert last["fin_cnt"][1] < K and done_at[1] == F.CHAIN_STEPS - 1 and last["n_cur"][1] == prm.n_max
    assert last["fin_cnt"][2] < K and last["n_past_w"][2] + 1 == prm.n_text_ctx and done_at[2] == 10
    # timestamp pairs run through window 1's beams
    assert any((o["tokens"][K:2 * K, :o["n_cur"][1]] >= vo.ts_begin).sum(axis=1).max() >= 2 for _, _, o in infos)
