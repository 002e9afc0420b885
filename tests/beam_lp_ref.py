"""float64 reference of what ohw_beam_search_ex adds to a beam search, on top of tests/beam_ref.py (imported, not edited):

  step_lp       one step's per-token log-probability bookkeeping (beam_update_kernel with plog set): plog_next / fin_plog follow
                from the step's sources, chosen candidates and pool slots
  nosp_prob     the no-speech probability of a first step's row (soft-max of the biased, unfiltered row)
  final_pick    the final ranking over a candidate list (the published decoder's finalize() + the best sum per token)
  finish        the same from a pool and live state in the device's layout, with tokens and log-probabilities copied out
                (beam_finish_kernel, ohw_beam_finish_host)
  finish_cases  crafted pools and live states; test_beam_finish_cpu.py checks their score gaps, test_gpu_beam_logprobs.py
                runs them on the device

No device, no torch."""
import numpy as np

import beam_ref as R

SENT_I, SENT_F, NEG = R.SENT_I, float(R.SENT_F), R.NEG


def step_lp(vo, prm, K, first, st, logits, bias=None):
    """R.step plus the history: st holds plog and fin_plog [R][max_tokens + 1] next to R.new_state's keys.
    -> (out, info): R.step's, out with plog (= plog_next) and fin_plog; what the device does not write holds the sentinel
    (plog_next everywhere else, fin_plog's rows from the input's fin_cnt on) or its input (the used pool rows)."""
    base = {k: v for k, v in st.items() if k not in ("plog", "fin_plog")}
    out, info = R.step(vo, prm, K, first, base, logits, bias)
    W = st["n_cur"].size
    Rn, L = W * K, prm.max_tokens + 1
    plog = np.asarray(st["plog"], np.float64).reshape(Rn, L)
    nxt = np.full((Rn, L), SENT_F)
    fin = np.array(st["fin_plog"], np.float64).reshape(Rn, L)
    for w in range(W):
        fin[w * K + int(st["fin_cnt"][w]):(w + 1) * K] = SENT_F
        if st["win_done"][w]:
            continue
        n = int(st["n_cur"][w])
        # the step's ranking, walked again on R.step's own candidates in R.step's order (score descending; the earlier beam, then
        # the earlier candidate): which source and which candidate every new beam and every new pool entry came from.  Each
        # decision is checked against what R.step wrote.
        cands = []
        for j in range(1 if first else K):
            r = w * K + j
            if not first and not st["beam_sum"][r] > NEG:
                continue
            b = 0.0 if first else float(st["beam_sum"][r])
            for c in range(K + 1):
                if out["cand_tok"][r, c] >= 0:
                    cands.append((b + float(out["cand_lp"][r, c]), j, c))
        cands.sort(key=lambda x: (-x[0], x[1], x[2]))
        saved, slot = 0, int(st["fin_cnt"][w])
        for score, j, c in cands:
            if saved >= K:
                break
            src, tok, own = w * K + j, int(out["cand_tok"][w * K + j, c]), float(out["cand_lp"][w * K + j, c])
            if tok == vo.eot:
                if slot < K:
                    f = w * K + slot
                    assert out["fin_sum"][f] == score and out["fin_len"][f] == n and np.array_equal(out["fin_tok"][f, :n], st["tokens"][src, :n])
                    fin[f, :n] = plog[src, :n]
                    fin[f, n] = own
                    slot += 1
            else:
                r_new = w * K + saved
                assert out["beam_sum"][r_new] == score and out["tokens"][r_new, n] == tok and np.array_equal(out["tokens"][r_new, :n], st["tokens"][src, :n])
                nxt[r_new, :n] = plog[src, :n]
                nxt[r_new, n] = own
                last = src
                saved += 1
        assert slot == out["fin_cnt"][w] and saved == info["saved"][w]
        # dead rows repeat the last live continuation's history (row 0's when there is none); their own value is -inf
        for j in range(saved, K):
            r_new = w * K + j
            src = last if saved else w * K
            assert not out["beam_sum"][r_new] > NEG and np.array_equal(out["tokens"][r_new, :n], st["tokens"][src, :n])
            nxt[r_new, :n] = plog[src, :n]
            nxt[r_new, n] = NEG
    out["plog"], out["fin_plog"] = nxt, fin
    return out, info


def nosp_prob(vo, logits_row, bias=None) -> float:
    v = np.asarray(logits_row, np.float32)
    if bias is not None:
        v = v + np.asarray(bias, np.float32)
    v = v.astype(np.float64)
    m = v.max()
    return float(np.exp(v[vo.nosp] - (m + np.log(np.exp(v - m).sum()))))


def final_pick(cands):
    """cands: [(tokens, sum)] in candidate order -> (index of the winner or -1, scores): sum / max(1, n), the first strict maximum"""
    best, best_score, scores = -1, NEG, []
    for i, (t, s) in enumerate(cands):
        score = s / max(1, len(t))
        scores.append(score)
        if best < 0 or score > best_score:
            best, best_score = i, score
    return best, scores


def finish(K, st, max_tokens=None):
    """st: fin_cnt / n_cur [W], fin_len / fin_sum / beam_sum [R], fin_tok / tokens [R][S], fin_plog / plog [R][S + 1].
    -> (out, info).  out: tokens [W][max_tokens], logprobs [W][max_tokens + 1] (sentinel where nothing is written), n_tokens,
    sum_logprob, ended_by_eot, n_finished [W].  info: per window the candidates' scores and the gap between the best two."""
    W = int(np.asarray(st["n_cur"]).size)
    S = int(np.asarray(st["tokens"]).shape[1])
    n_out = S if max_tokens is None else max_tokens
    out = dict(tokens=np.full((W, n_out), SENT_I, np.int32), logprobs=np.full((W, n_out + 1), SENT_F), n_tokens=np.zeros(W, np.int32),
               sum_logprob=np.zeros(W), ended_by_eot=np.zeros(W, np.int32), n_finished=np.zeros(W, np.int32))
    info = dict(scores=[], gap=np.full(W, np.inf), n_cand=np.zeros(W, np.int32))
    for w in range(W):
        n_cur = int(st["n_cur"][w])
        cands = []          # (tokens, sum, from_pool, row)
        for f in range(int(st["fin_cnt"][w])):
            r = w * K + f
            cands.append(([int(t) for t in st["fin_tok"][r, :st["fin_len"][r]]], float(st["fin_sum"][r]), 1, r))
        if len(cands) < K:
            sums = [float(st["beam_sum"][w * K + j]) for j in range(K)]
            for j in sorted(range(K), key=lambda j: -sums[j]):        # sorted() is stable
                if len(cands) >= K:
                    break
                if sums[j] > NEG:
                    cands.append(([int(t) for t in st["tokens"][w * K + j, :n_cur]], sums[j], 0, w * K + j))
        best, scores = final_pick([(c[0], c[1]) for c in cands])
        info["scores"].append(scores)
        info["n_cand"][w] = len(cands)
        top = sorted(scores, reverse=True)
        if len(top) >= 2:
            info["gap"][w] = top[0] - top[1]
        out["n_finished"][w] = int(st["fin_cnt"][w])
        if best < 0:
            continue
        t, s, pool, r = cands[best]
        n = min(len(t), n_out)
        lp = np.asarray(st["fin_plog"] if pool else st["plog"], np.float64)[r]
        out["tokens"][w, :n] = t[:n]
        out["logprobs"][w, :n] = lp[:n]
        if pool:
            out["logprobs"][w, n] = lp[len(t)]
        out["n_tokens"][w], out["sum_logprob"][w], out["ended_by_eot"][w] = n, s, pool
    return out, info


# ------------------------------------------------------------------------------------------------ crafted finish cases
def _fill(st, K, w, pool=(), live=(), n_cur=0):
    """pool: [(n, sum)], live: [sum] * K; tokens and log-probabilities are distinct per (row, position): a copy from the wrong row
    or position shows as another token / a value whole units off"""
    S = st["tokens"].shape[1]
    st["fin_cnt"][w], st["n_cur"][w] = len(pool), n_cur
    for f, (n, s) in enumerate(pool):
        r = w * K + f
        st["fin_len"][r], st["fin_sum"][r] = n, s
        st["fin_tok"][r, :n] = 1000 + 37 * r + np.arange(n)
        st["fin_plog"][r, :n + 1] = -(r + 1 + np.arange(n + 1) / 1000.0)
    for j, s in enumerate(live):
        r = w * K + j
        st["beam_sum"][r] = s
        st["tokens"][r, :n_cur] = 20000 + 41 * r + np.arange(n_cur)
        st["plog"][r, :n_cur] = -(100 + r + np.arange(n_cur) / 1000.0)


def finish_cases(K, S=448):
    """-> [(name, state, max_tokens, tie)]: one window each, plus one state that holds them all as windows of one launch"""
    def new(W):
        Rn = W * K
        return dict(fin_cnt=np.zeros(W, np.int32), fin_len=np.zeros(Rn, np.int32), fin_sum=np.zeros(Rn), fin_tok=np.full((Rn, S), 7, np.int32),
                    fin_plog=np.full((Rn, S + 1), -55.0), n_cur=np.zeros(W, np.int32), tokens=np.full((Rn, S), 9, np.int32),
                    plog=np.full((Rn, S + 1), -66.0), beam_sum=np.zeros(Rn))
    perm = {2: [1, 0], 3: [2, 0, 1], 5: [3, 0, 4, 1, 2]}[K]
    live_d = [-4.0 - 0.7 * perm[j] for j in range(K)]                       # not sorted by beam index: beam 1 is the best
    specs = [
        # the pool is full: the live beams (better per token) must not be looked at
        ("pool_full", dict(pool=[(4 + f, -2.0 - 1.3 * ((2 * f + 1) % K)) for f in range(K)], live=[-0.1] * K, n_cur=10), None, False),
        # one pool entry, K - 1 live beams join in sum order; the best live beam (not beam 0) wins
        ("pool_part", dict(pool=[(5, -6.0)], live=live_d, n_cur=8), None, False),
        ("pool_empty", dict(pool=[], live=live_d, n_cur=12), None, False),
        # a dead beam with the best place by index is skipped
        ("dead_live", dict(pool=[], live=[NEG] + [-3.0 - 0.4 * j for j in range(K - 1)], n_cur=6), None, False),
        ("all_dead_pool_one", dict(pool=[(3, -2.5)], live=[NEG] * K, n_cur=6), None, False),
        # end-of-text first: length 0, the divisor is max(1, 0)
        ("len0_wins", dict(pool=[(0, -0.4), (6, -6.0)], live=[-5.0 - j for j in range(K)], n_cur=7), None, False),
        ("len0_loses", dict(pool=[(0, -3.0), (6, -6.0)], live=[-50.0 - j for j in range(K)], n_cur=7), None, False),
        # the winner is longer than max_tokens: clipped
        ("clipped", dict(pool=[(40, -8.0), (3, -9.0)], live=[-90.0 - j for j in range(K)], n_cur=41), 16, False),
        ("clipped_live", dict(pool=[], live=[-20.0 - 3 * j for j in range(K)], n_cur=50), 16, False),
        # equal scores (-6 / 4 = -3 / 2 exactly): the earlier candidate wins
        ("tie_pool", dict(pool=[(4, -6.0), (2, -3.0)], live=[-80.0 - j for j in range(K)], n_cur=9), None, True),
        ("tie_pool_live", dict(pool=[(4, -6.0)], live=[-40.0] * (K - 1) + [-15.0], n_cur=10), None, True),
        # two live beams with the same sum (their tokens differ): the lower beam index joins first and wins
        ("tie_live", dict(pool=[], live=[-30.0] * (K - 2) + [-7.0, -7.0], n_cur=5), None, True),
        ("nothing", dict(pool=[], live=[NEG] * K, n_cur=3), None, False),
    ]
    cases = []
    for name, kw, mt, tie in specs:
        st = new(1)
        _fill(st, K, 0, **kw)
        cases.append((name, st, mt, tie))
    allw = new(len(specs))
    for w, (name, kw, mt, tie) in enumerate(specs):
        _fill(allw, K, w, **kw)
    cases.append(("all_windows", allw, None, True))
    return cases
