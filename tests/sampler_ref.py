"""numpy reference of ONE sampler call on ONE row (sampler_kernel, sampler_t_row and their shared update tail,
openhush_amd/csrc/decode.hip) in float64.  The logits filter and the timestamp-mass rule are beam_ref's (filter_row, pinned to
the oracle by test_beam_ref_cpu.py); this file adds the pick, the draw and the tail's state update.  No device, no torch.
Shared by test_sampler_ref_cpu.py (which pins it to the oracle) and test_gpu_sampler_rows.py.

Every decision carries the distance that makes a comparison with an fp32 implementation fair: `gap` between the two best
candidates of an arg-max, `ts_margin` of the timestamp-mass comparison, `edge` of a draw's target to the nearer boundary of the
picked token's interval of the cumulative distribution.

force_len (ohw_sample_params; not part of beam_ref.Params, the beam search refuses it) is a keyword: below its length
end-of-text is suppressed, and it replaces n_max in the update."""
import collections

import numpy as np

from beam_ref import NEG, SENT_F, SENT_I, Params, Vocab, allowed_mask, filter_row, vocab_layout     # noqa: F401 (re-exported)

EOT = 50257                 # vocab_layout's end-of-text: the same id in both vocabularies

Greedy = collections.namedtuple("Greedy", "token lp nosp gap ts_margin forced")
Draw = collections.namedtuple("Draw", "token lp nosp edge ts_margin forced")


def _biased(logits, bias) -> np.ndarray:
    v = np.asarray(logits, dtype=np.float32)
    if bias is not None:
        with np.errstate(invalid="ignore"):
            v = v + np.asarray(bias, dtype=np.float32)        # one fp32 addition, as on the device
    return v.astype(np.float32)


def _no_speech(vo: Vocab, v: np.ndarray, hist):
    """softmax of the UNFILTERED row at nosp; defined for an empty history only.  -inf entries weigh 0"""
    if len(hist):
        return None
    x = v.astype(np.float64)
    m = x.max()
    return float(np.exp(x[vo.nosp] - m) / np.exp(x - m).sum())


def _filtered(vo: Vocab, prm: Params, v: np.ndarray, hist, force_len: int):
    if force_len > 0 and len(hist) < force_len:
        v = v.copy()
        v[vo.eot] = NEG                 # filter_row drops -inf entries: suppressed
    return filter_row(vo, prm, v, None, hist)


def greedy(vo: Vocab, prm: Params, logits, bias, hist, force_len: int = 0) -> Greedy:
    """The arg-max over the allowed set (timestamps only when the mass rule forces them), the lowest index among equal values.
    gap: the distance between the two best values that compete (0: an exact tie; inf: one candidate)."""
    v = _biased(logits, bias)
    lp, margin, forced = _filtered(vo, prm, v, hist, force_len)
    tok = int(np.argmax(lp))            # the first of equal maxima
    assert lp[tok] > NEG, "nothing is allowed"
    rest = np.delete(lp, tok)
    second = rest.max()
    gap = float(lp[tok] - second) if second > NEG else np.inf
    return Greedy(tok, float(lp[tok]), _no_speech(vo, v, hist), gap, margin, forced)


def scaled(logits, bias, T) -> np.ndarray:
    """v = fl32(fl32(logit + bias) / fl32(T)): the two fp32 operations of the device and of ohw_sample_host"""
    with np.errstate(invalid="ignore"):
        return (_biased(logits, bias) / np.float32(T)).astype(np.float32)


def distribution(vo: Vocab, prm: Params, logits, bias, hist, T, force_len: int = 0):
    """-> (lp float64 [V] over what is allowed (text dropped when forced), cp: running sum of exp(lp), nosp, ts_margin, forced)"""
    v = scaled(logits, bias, T)
    lp, margin, forced = _filtered(vo, prm, v, hist, force_len)
    cp = np.cumsum(np.exp(lp))          # exp(-inf) = 0
    return lp, cp, _no_speech(vo, v, hist), margin, forced


def pick(cp: np.ndarray, u: float):
    """the first i with cp[i] >= u * cp[-1] -> (i, edge).  edge: distance of the target to the nearer end of i's interval,
    divided by the total.  An end counts only where another pick lies beyond it: with no probability below the interval every
    positive target lands in it or later whatever the rounding, and likewise above the last token that has any."""
    total = cp[-1]
    target = u * total
    i = int(np.searchsorted(cp, target, side="left"))
    assert i < cp.size and cp[i] > 0.0
    lo = cp[i - 1] if i else 0.0
    ends = []
    if lo > 0.0:
        ends.append(target - lo)
    if cp[i] < total:
        ends.append(cp[i] - target)
    return i, (float(min(ends) / total) if ends else np.inf)


def midpoint(cp: np.ndarray, i: int) -> float:
    """the u that aims at the middle of token i's interval"""
    lo = cp[i - 1] if i else 0.0
    return float(0.5 * (lo + cp[i]) / cp[-1])


def draw(vo: Vocab, prm: Params, logits, bias, hist, T, u, force_len: int = 0) -> Draw:
    lp, cp, nosp, margin, forced = distribution(vo, prm, logits, bias, hist, T, force_len)
    i, edge = pick(cp, u)
    return Draw(i, float(lp[i]), nosp, edge, margin, forced)


# ------------------------------------------------------------------------------------------------ the update tail
def new_row(prm: Params, hist, n_past=0, done=0, sum_logprob=0.0) -> dict:
    """one row of sampler state as ohw_dbg_sample_ex prepares it: the sentinel in next_tok, in the whole tok_lp row and in the
    history slot at n_cur"""
    n = len(hist)
    assert 0 <= n < prm.max_tokens
    tokens = np.zeros(prm.max_tokens, np.int32)
    tokens[:n] = hist
    tokens[n] = SENT_I
    return dict(tokens=tokens, n_cur=n, n_past=int(n_past), done=int(done), sum_logprob=float(sum_logprob), next_tok=SENT_I,
                tok_lp=np.full(prm.max_tokens + 1, float(SENT_F)))


def update(prm: Params, row: dict, token: int, lp: float, advance: int, force_len: int = 0):
    """the tail's rule for one row -> (the row afterwards, 1 if it finished in this call else 0)"""
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in row.items()}
    if row["done"]:
        return out, 0
    n_cur, np_now = row["n_cur"], row["n_past"] + advance
    n_max = force_len if force_len > 0 else prm.n_max
    out["tok_lp"][n_cur] = lp
    out["next_tok"] = int(token)
    finished = False
    if token == EOT:
        finished = True
    else:
        out["tokens"][n_cur] = token
        out["n_cur"] = n_cur + 1
        out["sum_logprob"] = row["sum_logprob"] + lp
        if advance:
            out["n_past"] = np_now
        finished = n_cur + 1 >= n_max or n_cur + 1 >= prm.max_tokens or np_now + 1 >= prm.n_text_ctx
    if finished:
        out["done"] = 1
    return out, int(finished)
