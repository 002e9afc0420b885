"""The final ranking of a beam search and the per-token log-probability bookkeeping, on the host: no GPU.

1. tests/beam_lp_ref.py's float64 finish rule is pinned two ways: to the oracle (on micro windows the oracle's winner is the
   rule applied to the oracle's own candidate list) and to ohw_beam_finish_host (crafted pools and live states: tokens,
   lengths, flags exactly; log-probabilities and sums are copies of fp32-exact inputs, so exactly too).
2. Except for the deliberate ties, every crafted case keeps its best and second-best scores at least 1e-3 apart, so an fp32
   implementation owes the same winner (scores are sums below 100 in magnitude over at most 50 tokens: one fp32 division's
   rounding is below 1e-5).
3. The reference of one step's bookkeeping (step_lp) is consistent with the step reference it stands on: along a chained run
   the history of every live beam and of every pool entry sums to its cumulative score."""
import numpy as np
import pytest

import beam_fixtures as F
import beam_lp_ref as L
import beam_ref as R
from openhush_amd import synth


@pytest.fixture(scope="module")
def E():
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


def test_finish_reference_picks_the_oracles_winner(oracle, tmp_models):
    om = oracle.Model.load(tmp_models("micro"))
    op = om.default_params(); op.n_max = 24
    seen_live = seen_pool = 0
    for seed in (3, 11):
        enc = om.encode(om.log_mel(synth.synth_audio(seed), 0))
        for K, bias in ((5, _bias(om, 6.0, 27.0)), (3, _bias(om, 8.0, 26.0)), (2, None)):
            ref = oracle.beam_search(om, enc, op, K, bias)
            best, scores = L.final_pick(ref["candidates"])
            assert best >= 0 and ref["candidates"][best][0] == ref["tokens"], (seed, K, ref)
            assert abs(ref["candidates"][best][1] - ref["sum_logprob"]) < 1e-6
            assert len(ref["candidates"]) <= K
            seen_pool += ref["n_finished"] > 0
            seen_live += ref["n_finished"] < K
    assert seen_pool and seen_live


@pytest.mark.parametrize("K", [2, 3, 5])
def test_crafted_cases_keep_their_scores_apart(K):
    names = set()
    for name, st, mt, tie in L.finish_cases(K, S=64):
        out, info = L.finish(K, st, mt)
        names.add(name)
        if name == "all_windows":
            continue
        if tie:
            assert info["gap"][0] == 0.0, (name, info)
            rest = sorted(set(info["scores"][0]), reverse=True)
            assert len(rest) < 2 or rest[0] - rest[1] >= 1e-3
        elif info["n_cand"][0] >= 2:
            assert info["gap"][0] >= 1e-3, (name, info)
        # what each case is there for
        if name == "pool_full":
            assert info["n_cand"][0] == K and out["ended_by_eot"][0] == 1
        if name == "pool_part":
            assert info["n_cand"][0] == K and out["ended_by_eot"][0] == 0 and out["tokens"][0, 0] == 20000 + 41 * 1
        if name == "pool_empty":
            assert out["n_finished"][0] == 0 and out["tokens"][0, 0] == 20000 + 41 * 1 and out["n_tokens"][0] == 12
        if name == "dead_live":
            assert info["n_cand"][0] == K - 1 and out["tokens"][0, 0] == 20000 + 41 * 1
        if name == "all_dead_pool_one":
            assert info["n_cand"][0] == 1 and out["ended_by_eot"][0] == 1
        if name == "len0_wins":
            assert out["n_tokens"][0] == 0 and out["ended_by_eot"][0] == 1 and out["logprobs"][0, 0] == -1.0 and out["sum_logprob"][0] == -0.4
        if name == "len0_loses":
            assert out["n_tokens"][0] == 6 and out["ended_by_eot"][0] == 1
        if name == "clipped":
            assert out["n_tokens"][0] == 16 and out["tokens"].shape == (1, 16) and out["logprobs"][0, 16] == -(1 + 40 / 1000.0)
        if name == "clipped_live":
            assert out["n_tokens"][0] == 16 and out["ended_by_eot"][0] == 0 and out["logprobs"][0, 16] == L.SENT_F
        if name == "tie_pool":
            assert out["n_tokens"][0] == 4
        if name == "tie_pool_live":
            assert out["ended_by_eot"][0] == 1
        if name == "tie_live":
            assert out["tokens"][0, 0] == 20000 + 41 * (K - 2)
        if name == "nothing":
            assert info["n_cand"][0] == 0 and out["n_tokens"][0] == 0 and (out["tokens"] == L.SENT_I).all()
    assert {"pool_full", "pool_part", "pool_empty", "dead_live", "len0_wins", "clipped", "tie_pool", "tie_live", "nothing", "all_windows"} <= names


def _same(got, want, what):
    for k in ("tokens", "n_tokens", "ended_by_eot", "n_finished"):
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    # copies of values that fp32 holds exactly
    assert np.array_equal(got["logprobs"], want["logprobs"].astype(np.float32)), (what, got["logprobs"], want["logprobs"])
    assert np.array_equal(got["sum_logprob"], want["sum_logprob"].astype(np.float32)), (what, got["sum_logprob"], want["sum_logprob"])


@pytest.mark.parametrize("K", [2, 3, 5])
def test_host_twin_matches_the_reference(E, K):
    for S in (64, 448):
        for name, st, mt, tie in L.finish_cases(K, S=S):
            want, _ = L.finish(K, st, mt)
            _same(E.beam_finish_host(K, st, mt), want, f"K={K} S={S} {name}")
    # max_tokens 0: lengths and flags only
    name, st, mt, tie = L.finish_cases(K, S=64)[0]
    got = E.beam_finish_host(K, st, 0)
    assert got["n_tokens"][0] == 0 and got["tokens"].shape == (1, 0) and got["ended_by_eot"][0] == 1


def test_host_twin_checks_its_arguments(E):
    K = 3
    name, st, mt, tie = L.finish_cases(K, S=64)[0]

    def bad(key, idx, value, K_=K, mt_=None):
        s2 = {k: np.array(a, copy=True) for k, a in st.items()}
        if key:
            s2[key][idx] = value
        with pytest.raises(E.WhisperError) as ex:
            E.beam_finish_host(K_, s2, mt_)
        assert ex.value.code == E.OHW_E_INVALID_ARG

    bad("fin_cnt", 0, K + 1)
    bad("fin_cnt", 0, -1)
    bad("fin_len", 1, 65)
    bad("n_cur", 0, 65)
    bad("n_cur", 0, -1)
    bad(None, 0, 0, mt_=65)
    bad(None, 0, 0, mt_=-1)
    for K_ in (1, 6):
        s2 = dict(fin_cnt=np.zeros(1, np.int32), fin_len=np.zeros(K_, np.int32), fin_sum=np.zeros(K_), fin_tok=np.zeros((K_, 64), np.int32),
                  fin_plog=np.zeros((K_, 65)), n_cur=np.ones(1, np.int32), tokens=np.zeros((K_, 64), np.int32), plog=np.zeros((K_, 65)),
                  beam_sum=np.zeros(K_))
        with pytest.raises(E.WhisperError):
            E.beam_finish_host(K_, s2)


@pytest.mark.parametrize("V", [51865, 51866])
def test_step_bookkeeping_sums_to_the_cumulative_scores(V):
    """the chained fixture of test_gpu_beam_step.py with a history: every live beam's and every pool entry's values sum to its
    score, and the -inf of a dead row sits at its last position"""
    vo = R.vocab_layout(V, 220)
    prm = F.chain_params(vo)
    K, W = F.CHAIN_K, F.CHAIN_W
    Ln = prm.max_tokens + 1
    hist = {"plog": np.zeros((W * K, Ln)), "fin_plog": np.zeros((W * K, Ln))}
    dead = pooled = 0

    def stepper(first, st, lg, side):
        out, _ = L.step_lp(vo, prm, K, first, dict(st, **hist), lg, None)
        hist["plog"], hist["fin_plog"] = out.pop("plog"), out.pop("fin_plog")
        return out

    was_done = np.zeros(W, np.int32)
    for s, st in F.run_chain(vo, stepper):
        for w in range(W):
            if was_done[w]:             # a finished window's rows are not written: the other half holds nothing of it
                continue
            n = int(st["n_cur"][w])
            for j in range(K):
                r = w * K + j
                if st["beam_sum"][r] > -np.inf:
                    assert abs(hist["plog"][r, :n].sum() - st["beam_sum"][r]) < 1e-9 and hist["plog"][r, n] == L.SENT_F
                elif n and hist["plog"][r, n - 1] == -np.inf:
                    dead += 1
            for f in range(int(st["fin_cnt"][w])):
                r = w * K + f
                m = int(st["fin_len"][r])
                assert abs(hist["fin_plog"][r, :m + 1].sum() - st["fin_sum"][r]) < 1e-9
                pooled += 1
            assert (hist["fin_plog"][w * K + int(st["fin_cnt"][w]):(w + 1) * K] == L.SENT_F).all()
        was_done = st["win_done"].copy()
    assert dead and pooled
