"""numpy reference of ONE beam step (beam_topk_kernel + beam_update_kernel, openhush_amd/csrc/decode.hip) in float64, in the
device's terms: the logits filter as the oracle's ref_process_logits_ex defines it, the K + 1 best allowed tokens of a row,
and the update as the oracle's ref_beam_search does it.  No device, no torch.  Shared by test_beam_ref_cpu.py (which pins it
to the oracle) and test_gpu_beam_step.py.

Every decision carries the gaps that make a comparison with an fp32 implementation fair: the smallest non-zero gap between
consecutive candidate log-probabilities of a row (the K + 2-th token counted), the smallest non-zero gap between the ranked
cumulative scores of a window, and the distance of the timestamp-mass comparison from its threshold."""
import collections

import numpy as np

SENT_I = -7777777          # OHW_DBG_SENTINEL_I32: what ohw_dbg_beam_step fills the output halves with
SENT_F = np.float32(-12345.0)
NEG = -np.inf

Vocab = collections.namedtuple("Vocab", "n_vocab eot sot translate transcribe solm prev nosp no_ts ts_begin blank n_langs")
# the sampling parameters and the limits a step reads (ohw_sample_params, the state's token capacity, the model's text context)
Params = collections.namedtuple("Params", "no_timestamps suppress_blank max_initial_ts n_max max_tokens n_text_ctx")


def vocab_layout(n_vocab: int, blank: int) -> Vocab:
    """whisper.cpp's special-token layout for a vocabulary size (multilingual: 51865 and 51866)"""
    assert n_vocab >= 51865
    n_langs = n_vocab - 51765 - 1
    dt = n_langs - 98
    return Vocab(n_vocab, 50257, 50258, 50357 + dt, 50358 + dt, 50359 + dt, 50360 + dt, 50361 + dt, 50362 + dt, 50363 + dt, blank, n_langs)


def default_params(n_max=220, no_timestamps=0, n_text_ctx=448) -> Params:
    return Params(no_timestamps, 1, 50, n_max, n_text_ctx, n_text_ctx)


def allowed_mask(vo: Vocab, prm: Params, hist) -> np.ndarray:
    """sp_allowed for every token of a row, given the tokens sampled so far in the window"""
    V, tb = vo.n_vocab, vo.ts_begin
    n = len(hist)
    ok = np.ones(V, dtype=bool)
    for t in (vo.no_ts, vo.sot, vo.nosp, vo.translate, vo.transcribe, vo.prev, vo.solm):
        ok[t] = False
    ok[vo.sot + 1:vo.sot + 1 + vo.n_langs] = False
    if n == 0 and prm.suppress_blank:
        ok[vo.eot] = False
        if vo.blank >= 0:
            ok[vo.blank] = False
    if prm.no_timestamps:
        ok[tb:] = False
        return ok
    last_ts = n > 0 and hist[n - 1] >= tb
    penult_ts = n < 2 or hist[n - 2] >= tb
    if last_ts:
        if penult_ts:
            ok[tb:] = False
        else:
            ok[:vo.eot] = False
    if n == 0 and prm.max_initial_ts > 0:
        ok[tb + prm.max_initial_ts + 1:] = False
    seen = [t for t in hist if t >= tb]
    if seen:
        ok[tb:seen[-1]] = False           # timestamps do not decrease
    return ok


def _lse(x: np.ndarray) -> float:
    m = x.max()
    return float(m + np.log(np.exp(x - m).sum()))


def filter_row(vo: Vocab, prm: Params, logits, bias, hist):
    """-> (lp float64 [V]: log-probabilities over the allowed set, -inf elsewhere; no renormalisation after the timestamp-mass
    rule, ts_margin: |log timestamp mass - best text log-probability| or inf where the rule does not apply, forced)"""
    v = np.asarray(logits, dtype=np.float32)
    if bias is not None:
        v = v + np.asarray(bias, dtype=np.float32)        # an fp32 addition, on the device and in the oracle alike
    v = v.astype(np.float64)
    ok = allowed_mask(vo, prm, hist) & (v > NEG)
    lp = np.full(vo.n_vocab, NEG)
    if not ok.any():
        return lp, np.inf, False
    lse = _lse(v[ok])
    lp[ok] = v[ok] - lse
    margin, forced = np.inf, False
    ts, tx = lp[vo.ts_begin:], lp[:vo.ts_begin]
    if not prm.no_timestamps and (ts > NEG).any():
        ts_lp = _lse(ts[ts > NEG])
        text_lp = tx.max()
        if text_lp > NEG:
            margin = abs(ts_lp - text_lp)
        if ts_lp > text_lp:
            forced = True
            lp[:vo.ts_begin] = NEG
    return lp, margin, forced


def top_candidates(lp: np.ndarray, K: int):
    """the K + 1 best tokens, the lowest index first among equal values -> (tok int32 [K + 1] (-1: none), lp float64 [K + 1]
    (-inf: none), gap: smallest non-zero gap between consecutive values of the K + 2 best)"""
    n = K + 2
    thr = np.partition(lp, lp.size - n)[lp.size - n]
    idx = np.flatnonzero((lp >= thr) & (lp > NEG))
    idx = idx[np.lexsort((idx, -lp[idx]))][:n]
    vals = lp[idx]
    d = -np.diff(vals)
    gap = float(d[d > 0].min()) if (d > 0).any() else np.inf
    tok = np.full(K + 1, -1, dtype=np.int32)
    out = np.full(K + 1, NEG)
    m = min(K + 1, idx.size)
    tok[:m] = idx[:m]
    out[:m] = vals[:m]
    return tok, out, gap


def new_state(W: int, K: int, prm: Params):
    """an all-zero state of W windows in the device's layout (float64 sums)"""
    R, MT, C = W * K, prm.max_tokens, prm.n_text_ctx
    return dict(tokens=np.zeros((R, MT), np.int32), kv_slot=np.zeros((R, C), np.int32), beam_sum=np.zeros(R, np.float64),
                n_cur=np.zeros(W, np.int32), n_past_w=np.zeros(W, np.int32), win_done=np.zeros(W, np.int32),
                fin_cnt=np.zeros(W, np.int32), fin_tok=np.zeros((R, MT), np.int32), fin_len=np.zeros(R, np.int32),
                fin_sum=np.zeros(R, np.float64))


def step(vo: Vocab, prm: Params, K: int, first: bool, st: dict, logits: np.ndarray, bias=None):
    """One beam step.  st: the state (new_state's keys); logits [W][V] when first, else [W * K][V].
    -> (out, info).  out: the complete next state - st's keys with tokens / kv_slot replaced by tokens_next / kv_slot_next, plus
    cand_tok, cand_lp, next_tok, n_past, n_done.  What the device does not write holds the sentinel (tokens_next, kv_slot_next,
    cand_*, next_tok, n_past, pool slots from fin_cnt on) or its input (everything else).
    info: per row cand_gap / ts_margin / forced, per window score_gap (all ranked candidates) / decided_gap (only the candidates
    the update loop looked at, and the first one it did not) / saved / n_live_in."""
    W = st["n_cur"].size
    R, MT, C = W * K, prm.max_tokens, prm.n_text_ctx
    K1 = K + 1
    out = {k: np.array(v, copy=True) for k, v in st.items()}
    out["beam_sum"] = out["beam_sum"].astype(np.float64)
    out["fin_sum"] = out["fin_sum"].astype(np.float64)
    tokens, kv = st["tokens"], st["kv_slot"]
    out["tokens"] = np.full((R, MT), SENT_I, np.int32)
    out["kv_slot"] = np.full((R, C), SENT_I, np.int32)
    out["cand_tok"] = np.full((R, K1), SENT_I, np.int32)
    out["cand_lp"] = np.full((R, K1), float(SENT_F))
    out["next_tok"] = np.full(R, SENT_I, np.int32)
    out["n_past"] = np.full(R, SENT_I, np.int32)
    for w in range(W):
        for f in range(int(st["fin_cnt"][w]), K):
            out["fin_tok"][w * K + f] = SENT_I
            out["fin_len"][w * K + f] = SENT_I
            out["fin_sum"][w * K + f] = float(SENT_F)
    info = dict(cand_gap=np.full(R, np.inf), ts_margin=np.full(R, np.inf), forced=np.zeros(R, bool),
                score_gap=np.full(W, np.inf), decided_gap=np.full(W, np.inf), saved=np.full(W, -1), n_live_in=np.full(W, -1))
    n_done = 0
    for w in range(W):
        if st["win_done"][w]:
            continue
        n_cur, P = int(st["n_cur"][w]), int(st["n_past_w"][w])
        # ---- top-k: every row of the window (the first step: its beam 0 alone, from the window's one logits row)
        for j in range(1 if first else K):
            r = w * K + j
            lp, margin, forced = filter_row(vo, prm, logits[w if first else r], bias, [int(t) for t in tokens[r, :n_cur]])
            out["cand_tok"][r], out["cand_lp"][r], info["cand_gap"][r] = top_candidates(lp, K)
            info["ts_margin"][r], info["forced"][r] = margin, forced
        # ---- update: rank the candidates of the live beams (score descending; ties: the earlier beam, then the earlier candidate)
        cands = []
        live = [j for j in range(1 if first else K) if first or st["beam_sum"][w * K + j] > NEG]
        info["n_live_in"][w] = len(live)
        for j in live:
            r = w * K + j
            base = 0.0 if first else float(st["beam_sum"][r])
            for c in range(K1):
                if out["cand_tok"][r, c] >= 0:
                    cands.append((base + float(out["cand_lp"][r, c]), j, c, int(out["cand_tok"][r, c])))
        cands.sort(key=lambda x: (-x[0], x[1], x[2]))
        sc = np.array([x[0] for x in cands])
        d = -np.diff(sc)
        if (d > 0).any():
            info["score_gap"][w] = float(d[d > 0].min())
        saved, fin_cnt, seen = [], int(st["fin_cnt"][w]), 0
        for score, j, c, tok in cands:
            if len(saved) >= K:
                break
            seen += 1
            if tok == vo.eot:
                if fin_cnt < K:
                    slot = w * K + fin_cnt
                    out["fin_tok"][slot, :n_cur] = tokens[w * K + j, :n_cur]
                    out["fin_len"][slot] = n_cur
                    out["fin_sum"][slot] = score
                    fin_cnt += 1
            else:
                saved.append((j, tok, score))
        n_saved = len(saved)
        info["saved"][w] = n_saved
        # the gaps the loop's outcome depends on: between the candidates it looked at, and to the first one it did not
        dd = d[:seen]
        if (dd > 0).any():
            info["decided_gap"][w] = float(dd[dd > 0].min())
        # rows j >= saved are dead (sum -inf); the device repeats the last live continuation in them (beam 0 and end-of-text when
        # there is none)
        while len(saved) < K:
            saved.append((saved[n_saved - 1][0], saved[n_saved - 1][1], NEG) if n_saved else (0, vo.eot, NEG))
        for j, (src, tok, score) in enumerate(saved):
            r = w * K + j
            out["tokens"][r, :n_cur] = tokens[w * K + src, :n_cur]
            out["tokens"][r, n_cur] = tok
            out["kv_slot"][r, :P + 1] = w if first else kv[w * K + src, :P + 1]
            out["kv_slot"][r, P + 1] = r
            out["beam_sum"][r] = score
            out["next_tok"][r] = tok
            out["n_past"][r] = P + 1
        out["fin_cnt"][w] = fin_cnt
        out["n_cur"][w] = n_cur + 1
        out["n_past_w"][w] = P + 1
        if fin_cnt >= K or n_saved == 0 or n_cur + 1 >= prm.n_max or n_cur + 1 >= prm.max_tokens or P + 2 >= prm.n_text_ctx:
            out["win_done"][w] = 1
            n_done += 1
    out["n_done"] = n_done
    return out, info


def final_candidates(K: int, st: dict, w: int):
    """the final candidates of window w as ref_beam_search lists them: the finished pool, topped up with the live beams (most
    likely first) -> ([(tokens, sum)], index of the winner: the best sum per token, the first among equals)"""
    n_cur = int(st["n_cur"][w])
    cands = [([int(t) for t in st["fin_tok"][w * K + f, :st["fin_len"][w * K + f]]], float(st["fin_sum"][w * K + f]))
             for f in range(int(st["fin_cnt"][w]))]
    if len(cands) < K:
        sums = [float(st["beam_sum"][w * K + j]) for j in range(K)]
        for j in sorted(range(K), key=lambda j: -sums[j]):        # sorted() is stable
            if len(cands) >= K:
                break
            if sums[j] > NEG:
                cands.append(([int(t) for t in st["tokens"][w * K + j, :n_cur]], sums[j]))
    best, best_score = -1, NEG
    for i, (t, s) in enumerate(cands):
        score = s / max(1, len(t))
        if best < 0 or score > best_score:
            best, best_score = i, score
    return cands, best
