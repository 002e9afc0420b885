"""Confidence scores in numpy: the definitions of include/ohw.h (ohw_token_score / ohw_state_score), restated in float64 from the
definition and not from the library's code, and the rows the CPU and the GPU tests share.

score_row(x, n_vocab, eot, target) -> the five values of one raw logits row.  logit, top_id and top_logit are selections and are
compared as 32-bit words; the two log-sum-exp values are compared within lse_bound(), derived here from the reduction order
score.hip states and not from its output.  expected(case, fault=NAME) applies a deliberately wrong rule (FAULTS): the CPU test
shows that compare(), the comparison the GPU test makes, flags each of them on the shared cases.

The bound of a log-sum-exp.  u = 2^-24 is float32's unit roundoff.  score.hip's order: 256 threads; thread t folds its columns
(16-byte groups t, t + 256, ...: n_t = 4 * ceil(ceil(n_vocab / 4) / 256) columns at most) one by one into a running pair (m, s),
    mn = max(m, x);  s = s * exp(m - mn) + exp(x - mn);  m = mn;
then 6 xor-tree merges inside a wave, 3 merges over the 4 waves, for lse_all 1 more merge of (text, special), each
    mn = max(m1, m2);  s = s1 * exp(m1 - mn) + s2 * exp(m2 - mn);
and finally m + log(s).  Follow the mass exp(x_i - m) of one column i from the step it enters to the end:
  steps         at most n_t + 10 of them.  In each, its mass is multiplied by an exp (taken as good to 2 ulp = 4u relative;
                the host's and the device's expf are specified to 1 ulp), the product is rounded (u) and the sum is rounded (u):
                6u a step
  arguments     the argument of each exp is one rounded subtraction: an absolute error of u * |argument| in the exponent, a
                relative one in the mass.  The maxima only grow, so the arguments along the column's way telescope:
                (mn_entry - x_i) + (m_final - mn_entry) = m_final - x_i = d_i >= 0.  d_i * u in all
  so            s is off by at most u * (6 (n_t + 10) + D) relative, D = sum_i w_i d_i the mean of d under the weights
                w_i = exp(-d_i) / sum_j exp(-d_j) (computed below from the row, in float64) - and that is the absolute error of
                log(s)
  log           2 ulp of |log s|: 4u |log s|
  m + log(s)    one rounding of the result: u |lse|
    lse_bound = 1.01 * u * (6 (n_t + 10) + D + 4 |log s| + |lse|)        (1.01: the second-order terms)
At 1003 columns n_t = 4, at 51 866 columns n_t = 204: the fixed part is 5.0e-6 and 7.7e-5 (print_bounds()).
"""
import math

import numpy as np

U = 2.0 ** -24
THREADS = 256                  # token_score_kernel's workgroup
SENT_F = np.float32(-12345.0)  # OHW_DBG_SENTINEL_F32 / _I32: what ohw_dbg_token_score fills the output entries with
SENT_I = -7777777
POISON = np.float32(3.0e30)    # the padding columns n_vocab .. ld - 1: any of them read into a result wrecks it
FIELDS = ("logit", "lse_text", "lse_all", "top_id", "top_logit")
DTYPE = np.dtype([("logit", np.float32), ("lse_text", np.float32), ("lse_all", np.float32), ("top_id", np.int32), ("top_logit", np.float32)])
FAULTS = ("eot_in_lse_text", "last_column_dropped", "padding_read", "last_maximum_on_tie", "top_id_past_eot", "neighbour_target",
          "row_at_n_all_written", "row_at_p_minus_2_written", "bias_applied")
BIAS_FAULT = 0.75              # the logit bias the "bias_applied" fault adds to every other text column


def n_t(n_vocab):
    return 4 * math.ceil(math.ceil(n_vocab / 4) / THREADS)


def lse64(x):
    x = np.asarray(x, np.float64)
    m = float(x.max())
    return m + math.log(float(np.exp(x - m).sum()))


def lse_bound(x, n_vocab):
    """the bound above for the log-sum-exp over the columns x (float64 values of the fp32 row) of a row of n_vocab columns"""
    x = np.asarray(x, np.float64)
    d = float(x.max()) - x
    w = np.exp(-d)
    s = float(w.sum())
    D = float((w * d).sum()) / s
    return 1.01 * U * (6 * (n_t(n_vocab) + 10) + D + 4 * abs(math.log(s)) + abs(lse64(x)))


def print_bounds():
    for n_vocab, eot in ((1003, 900), (51866, 50257)):
        x = 3.0 * np.random.default_rng(5).standard_normal(n_vocab).astype(np.float32).astype(np.float64)
        print(f"score_ref: {n_vocab} columns: n_t = {n_t(n_vocab)}, fixed part {1.01 * U * 6 * (n_t(n_vocab) + 10):.3g}, "
              f"lse_all bound of a 3 N(0, 1) row {lse_bound(x, n_vocab):.3g}, lse_text {lse_bound(x[:eot], n_vocab):.3g}")


def score_row(x, n_vocab, eot, target, fault=None, ld_row=None):
    """the definition on one row, float64.  x: the row's first n_vocab columns (ld_row: the whole row with its padding, which only
    the padding_read fault looks at)"""
    x = np.asarray(x, np.float64)[:n_vocab]
    text = x[:eot + 1] if fault == "eot_in_lse_text" else x[:eot]
    full = x[:n_vocab - 1] if fault == "last_column_dropped" else x
    if fault == "padding_read":
        full = np.asarray(ld_row, np.float64)
    top_src = x if fault == "top_id_past_eot" else x[:eot]
    top = int(np.argmax(top_src))                                   # numpy's arg-max is the first maximum
    if fault == "last_maximum_on_tie":
        top = int(len(top_src) - 1 - np.argmax(top_src[::-1]))
    return dict(logit=float(x[target]), lse_text=lse64(text), lse_all=lse64(full), top_id=top, top_logit=float(x[top]))


# ---- cases: what ohw_dbg_token_score takes ----------------------------------------------------------------------------------

def seam_columns(n_vocab, eot):
    """column 0, eot - 1, eot, n_vocab - 1 and the first and last column on either side of every kind of seam of the work shape:
    a thread's 16-byte group (every multiple of 4), a wave's 64 groups (every multiple of 256), the workgroup's stride (every
    multiple of 1024), the ragged last group"""
    last_group = 4 * ((n_vocab - 1) // 4)
    cols = [0, 3, 4, 255, 256, 259, 260, 511, 512, 767, 768, 1023, 1024, 1027, 1028, eot - 4, eot - 1, eot, eot + 1, last_group - 1,
            last_group, n_vocab - 1]
    for k in (2, 17, n_vocab // 1024):
        cols += [1024 * k - 1, 1024 * k, 1024 * k + 255, 1024 * k + 256]
    return sorted({c for c in cols if 0 <= c < n_vocab})


def make_case(n_vocab, eot, ld, n_all, row0, n_prompt=4, cap=16, seed=0):
    """-> dict: logits f32 [batch * 8][ld] (3 N(0, 1); padding columns POISON), targets, n_all, and per row what was planted.
    Rows cycle through: a maximum planted on a seam column (a non-text one makes the row's largest value a non-text column), an
    exact tie between two text columns, nothing; the targets walk the seam columns too"""
    batch = len(n_all)
    rng = np.random.default_rng([n_vocab, batch, row0, seed])
    rows = batch * 8
    lg = (3.0 * rng.standard_normal((rows, ld))).astype(np.float32)
    lg[:, n_vocab:] = POISON
    seams = seam_columns(n_vocab, eot)
    text_seams = [c for c in seams if c < eot]
    targets = np.zeros(rows, np.int32)
    for m in range(rows):
        k = (m * 5 + seed * 3 + row0) % len(seams)
        targets[m] = seams[(k + 7) % len(seams)]
        kind = m % 3
        if kind == 0:
            lg[m, seams[k]] = np.float32(17.5)
            if seams[k] >= eot:                               # the text maximum below it, on a seam as well
                lg[m, text_seams[k % len(text_seams)]] = np.float32(15.25)
        elif kind == 1:
            a, b = text_seams[k % len(text_seams)], text_seams[(k + 3) % len(text_seams)]
            lg[m, a] = lg[m, b] = np.float32(16.125)
    return dict(n_vocab=n_vocab, eot=eot, ld=ld, batch=batch, logits=lg, targets=targets, n_all=np.asarray(n_all, np.int32), row0=row0,
                n_prompt=n_prompt, cap=cap)


def expected(case, fault=None):
    """-> (want: DTYPE-like float64 dict of arrays [batch][cap], written: bool [batch][cap]) by the definition (or a faulty one)"""
    B, cap, P, row0 = case["batch"], case["cap"], case["n_prompt"], case["row0"]
    nv, eot, lg = case["n_vocab"], case["eot"], case["logits"]
    want = {f: np.zeros((B, cap), np.float64) for f in FIELDS}
    written = np.zeros((B, cap), bool)
    for m in range(B * 8):
        b, j = divmod(m, 8)
        pos = row0 + j
        lo = P - 2 if fault == "row_at_p_minus_2_written" else P - 1
        hi = case["n_all"][b] + (1 if fault == "row_at_n_all_written" and case["n_all"][b] > 0 else 0)
        entry = pos - (P - 1)
        if not lo <= pos < hi or entry >= cap:
            continue
        if entry < 0:
            entry = cap - 1         # (the faulty rule has to write somewhere: an entry the true rule leaves alone at these sizes)
        row = lg[m]
        if fault == "bias_applied":
            row = row.copy()
            row[0:eot:2] += np.float32(BIAS_FAULT)
        tgt_row = lg[m + 1 if m + 1 < B * 8 else m - 1] if fault == "neighbour_target" else row
        s = score_row(row, nv, eot, int(case["targets"][m]), fault=fault, ld_row=row)
        s["logit"] = float(tgt_row[case["targets"][m]])
        for f in FIELDS:
            want[f][b, entry] = s[f]
        written[b, entry] = True
    return want, written


def as_device(want, written, guard=0):
    """what a device that computed `want` exactly would hand back: DTYPE [guard + batch * cap + guard], sentinels elsewhere"""
    B, cap = written.shape
    out = np.zeros(B * cap + 2 * guard, DTYPE)
    for f in FIELDS:
        out[f] = SENT_I if f == "top_id" else SENT_F
    body = out[guard:guard + B * cap].reshape(B, cap)
    for f in FIELDS:
        body[f][written] = want[f][written].astype(DTYPE[f])
    return out


def compare(case, got, guard=0):
    """got: DTYPE [guard + batch * cap + guard] as ohw_dbg_token_score returns it -> (list of complaints (empty: all is well),
    worst lse error / bound)"""
    want, written = expected(case)
    B, cap = written.shape
    bad = []
    got = np.asarray(got)
    sent = as_device(want, np.zeros_like(written), guard)
    body = got[guard:guard + B * cap].reshape(B, cap)
    for name, part in (("front guard", got[:guard]), ("back guard", got[guard + B * cap:])):
        if part.tobytes() != sent[:len(part)].tobytes():
            bad.append(f"{name} was written")
    worst = 0.0
    lg64 = case["logits"].astype(np.float64)
    for b in range(B):
        for e in range(cap):
            g = body[b, e]
            if not written[b, e]:
                if g.tobytes() != sent[0].tobytes():
                    bad.append(f"window {b} entry {e} was written: {g}")
                continue
            m = b * 8 + (e + case["n_prompt"] - 1 - case["row0"])
            for f in ("logit", "top_logit"):
                if np.float32(want[f][b, e]).view(np.uint32) != g[f].view(np.uint32):
                    bad.append(f"window {b} entry {e} {f}: {g[f]!r}, want {want[f][b, e]!r}")
            if int(g["top_id"]) != int(want["top_id"][b, e]):
                bad.append(f"window {b} entry {e} top_id: {g['top_id']}, want {int(want['top_id'][b, e])}")
            for f, cols in (("lse_text", case["eot"]), ("lse_all", case["n_vocab"])):
                lim = lse_bound(lg64[m, :cols], case["n_vocab"]) + abs(want[f][b, e]) * U      # + the restatement's own cast to fp32
                err = abs(float(g[f]) - want[f][b, e])
                if not err <= lim:                            # a NaN fails
                    bad.append(f"window {b} entry {e} {f}: {g[f]!r}, want {want[f][b, e]!r}, error {err:.3g} > bound {lim:.3g}")
                else:
                    worst = max(worst, err / lim)
    return bad, worst


# ---- the sequence and the word rule -------------------------------------------------------------------------------------------

def scores_from_logits(all_pos_logits, n_prompt, tokens, eot, n_vocab):
    """all_pos_logits [positions][n_vocab]: the raw logits of the sequence [prompt, tokens] at every position -> the scores of
    ohw_state_score's entries 0 .. len(tokens): position n_prompt - 1 + i predicts tokens[i], the last one end-of-text"""
    out = []
    for i in range(len(tokens) + 1):
        target = int(tokens[i]) if i < len(tokens) else eot
        out.append(score_row(all_pos_logits[n_prompt - 1 + i], n_vocab, eot, target))
    return out


def word_probs(logprob_text, starts):
    """openai-whisper's timing.py: a word's probability is the mean of its tokens' probabilities, float64"""
    lp = np.asarray(logprob_text, np.float64)
    cuts = [i for i in range(len(lp)) if i == 0 or starts[i]] + [len(lp)]
    return np.asarray([np.mean(np.exp(lp[a:b])) for a, b in zip(cuts[:-1], cuts[1:])], np.float64)
