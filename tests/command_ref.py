"""Command lists in numpy: the rule of include/ohw.h (ohw_state_set_command_table), restated from the definition and not from the
library's code, and the cases the CPU and the GPU tests share.

rule(phrases, penalty, history, n_cur, row) -> (the row after the rule, list_logprob or None).  The lowering is one float32
subtraction, so rows are compared as 32-bit words and not within a tolerance.  list_logprob is computed here in float64 and
compared within lp_tol(), which is derived below from the kernel's reduction shape and not from its output.
rule(..., fault=NAME) applies a deliberately wrong rule (FAULTS): the CPU test shows that the comparison the GPU test makes
flags each of them on the shared cases.

The tolerance of list_logprob.  u = 2^-24 is float32's unit roundoff.  The kernel computes, for the children and for all text
columns, M = the exact maximum, S = sum of expf(x - M), and then (Mc + logf(Sc)) - (Ma + logf(Sa)).
  a term        a = M - x >= 0 is rounded once (a * u absolute), expf is taken as good to 2 ulp (4u relative; the device's expf
                is specified to 1 ulp): the term's relative error is at most (a + 4) u.  Weighted by the term's share
                w = exp(-a) / S of the sum, the a * u parts add up to u * sum(w * a) = u * (H(w) - ln S) <= u * ln N, because
                ln w = -a - ln S, the entropy H(w) is at most ln N, and S >= 1 (the maximum's own term is 1)
  the sum       1024 threads stride over N columns: ceil(N / 1024) sequential adds per thread, 6 shuffle levels within a wave,
                15 sequential adds over the 16 waves; all terms are positive, so each add costs at most u relative
  so            S is off by at most (4 + ln N + ceil(N / 1024) + 21) u relative, which is the absolute error of ln S
  logf          2 ulp of a result of at most ln N: 4u * ln N absolute
  M + logf(S)   one rounding of a value of magnitude at most L + ln N, L = max |logit|
  the two       each log-sum-exp carries all of the above; their difference is rounded once more, at most 2L + ln N in magnitude
    lp_tol(N, L) = u * (2 * (4 + ln N + ceil(N / 1024) + 21 + 4 ln N + L + ln N) + 2L + ln N)
For N = 900, L = 20: 1.3e-5.  For N = 50257, L = 20: 2.2e-5.  A row with -inf among its columns has fewer terms: the bound holds.
"""
import math

import numpy as np

BAN = np.float32(-1.0e30)      # OHW_REPEAT_BAN
MAX_LEN = 16
FAULTS = ("eot_free_mid_phrase", "eot_penalised_at_terminal", "child_penalised", "timestamp_penalised", "tail_match",
          "timestamps_not_skipped", "off_list_text_free", "reads_n_cur", "penalty_twice")

N_VOCAB, LD, MAX_TOKENS = 1003, 1024, 448
EOT = 900                      # text tokens are 0 .. 899; 900 is end-of-text, 901 .. 1002 stand for the special and timestamp ids
TS, TS2 = 950, 951             # two timestamp ids
SENTINEL = np.float32(-12345.678)     # guard columns, the guard row, list_logprob entries nobody writes
L_MAX = 20.0                   # the rows' logits are 3 * N(0, 1) and planted values below 20 in magnitude
THREADS = 1024                 # command_rule_kernel's workgroup


def lp_tol(n_text, l_max=L_MAX):
    u = 2.0 ** -24
    ln_n = math.log(max(n_text, 2))
    one = 4 + ln_n + math.ceil(n_text / THREADS) + 21 + 4 * ln_n + l_max + ln_n
    return u * (2 * one + 2 * l_max + ln_n)


def lse64(x):
    x = np.asarray(x, np.float64)
    x = x[x > -np.inf]
    if x.size == 0:
        return -math.inf
    m = float(x.max())
    return m + math.log(float(np.exp(x - m).sum()))


def rule(phrases, penalty, history, n_cur, row, eot=EOT, fault=None):
    """history: the row's buffer [max_tokens] (entries at and behind n_cur are not the row's history).  Returns (a new row,
    list_logprob in float64 when the history holds no text token, else None)"""
    out = np.array(row, dtype=np.float32, copy=True)
    n_vocab = out.size
    lim = min(eot, n_vocab)
    hist = [int(x) for x in history]
    h = hist[:n_cur + 1] if fault == "reads_n_cur" else hist[:n_cur]
    t = list(h) if fault == "timestamps_not_skipped" else [x for x in h if 0 <= x < eot]
    phrases = [tuple(int(x) for x in p) for p in phrases]
    prefixes = {p[:d] for p in phrases for d in range(len(p) + 1)}
    node = tuple(t) if len(t) <= MAX_LEN and tuple(t) in prefixes else None
    if fault == "tail_match" and node is None:
        for k in range(min(len(t), MAX_LEN), -1, -1):       # the longest tail that is a prefix; the empty one always is
            if tuple(t[len(t) - k:]) in prefixes:
                node = tuple(t[len(t) - k:])
                break
    children = set() if node is None else {p[len(node)] for p in phrases if len(p) > len(node) and p[:len(node)] == node}
    terminal = node is not None and node in set(phrases)
    p32 = np.float32(penalty)

    def lower(x):
        if np.isinf(p32):
            return BAN
        y = np.float32(x - p32)
        return np.float32(y - p32) if fault == "penalty_twice" else y

    lp = None
    if len(t) == 0:
        ch = [out[c] for c in sorted(children) if c < lim]
        lc = lse64(ch)
        lp = -math.inf if lc == -math.inf else lc - lse64(out[:lim])
    if node is None and fault == "off_list_text_free":
        return out, lp
    spare = set(children)
    if fault == "child_penalised" and spare:
        spare.discard(min(spare))
    with np.errstate(over="ignore", invalid="ignore"):
        for c in range(lim):
            if c not in spare:
                out[c] = lower(out[c])
        eot_lowered = node is not None and not terminal
        if fault == "eot_free_mid_phrase":
            eot_lowered = False
        if fault == "eot_penalised_at_terminal":
            eot_lowered = node is not None
        if eot_lowered and eot < n_vocab:
            out[eot] = lower(out[eot])
        if fault == "timestamp_penalised" and TS < n_vocab:
            out[TS] = lower(out[TS])
    return out, lp


# ---- the shared lists ------------------------------------------------------------------------------------------------------
LONG = list(range(30, 46))                                   # 16 tokens
LIST_A = ([[10], [20, 21], [20, 21, 22], LONG, [20, 21], [60, 61, 62]] +
          [[t] for t in range(100, 400)])                    # a root with 304 children; depth 1 holds 304 nodes
LIST_B = [[a, b] for a in range(500, 532) for b in range(600, 632)]      # 1024 phrases: depth 2 holds 1024 nodes
LIST_C = [[10], [20, 21]]                                    # two root children


# ---- the shared cases ------------------------------------------------------------------------------------------------------
def _case(tokens, poison=None, done=0, logits=None):
    """-> (history buffer, n_cur, done, {column: logit} to plant in the row); poison: what follows the row's tokens in its buffer
    (tokens that would change the node if they were read), else zeros"""
    h = np.zeros(MAX_TOKENS, np.int32)
    n = len(tokens)
    h[:n] = tokens
    if poison is not None and n < MAX_TOKENS:
        h[n:] = np.resize(np.atleast_1d(np.asarray(poison, np.int32)), MAX_TOKENS - n)
    return h, n, done, logits or {}


def cases_a():
    ninf = -np.inf
    full = [TS] * MAX_TOKENS
    full[100], full[300] = 20, 21
    return {
        "empty": _case([], poison=20),
        "timestamp only": _case([TS], poison=[20, 21]),
        "two timestamps, -inf columns": _case([TS, TS2], logits={5: ninf, 10: ninf, 150: ninf, 899: ninf}),
        "mid phrase behind a timestamp": _case([TS, 20]),
        "mid phrase, poison behind n_cur": _case([20], poison=21),
        "prefix of another, timestamps between": _case([20, TS, 21, TS2]),
        "whole phrase": _case([20, 21, 22], logits={EOT: 3.0, 22: 19.0}),
        "one token phrase": _case([10]),
        "depth 15": _case(LONG[:15]),
        "depth 16": _case([TS] + LONG + [TS2]),
        "17 text tokens": _case(LONG + [46]),
        "17 text tokens of a listed start": _case(LONG + [30]),
        "off the list": _case([11], logits={EOT: 4.0}),
        "listed tail behind an unlisted token": _case([11, 20]),
        "first of 304": _case([100]),
        "inside 304": _case([TS, 251]),
        "last of 304": _case([399]),
        "behind the 304": _case([400]),
        "n_cur = max_tokens": _case(full),
        "done": _case([20], done=1),
        "-inf child": _case([20], logits={21: ninf, 7: ninf}),
    }


def cases_b():
    return {
        "empty": _case([]),
        "first of 1024": _case([500, 600]),
        "inside 1024": _case([TS, 517, TS2, 613]),
        "last of 1024": _case([531, 631]),
        "not among 1024": _case([517, 599]),
        "depth 1 of 32": _case([531], poison=600),
        "three tokens": _case([500, 600, 600]),
    }


def cases_c():
    ninf = -np.inf
    return {
        "all children -inf": _case([], logits={10: ninf, 20: ninf}),
        "one child -inf": _case([TS], logits={10: ninf, 20: 2.5}),
        "every text column -inf": _case([], logits={c: ninf for c in range(EOT)}),
        "mid": _case([20]),
    }


def groups():
    """(name, phrases, penalty, cases)"""
    return [("A p=7.5", LIST_A, 7.5, cases_a()), ("A p=inf", LIST_A, math.inf, cases_a()), ("B p=100", LIST_B, 100.0, cases_b()),
            ("C p=1000", LIST_C, 1000.0, cases_c()), ("C p=inf", LIST_C, math.inf, cases_c())]


def make_rows(cases, seed, n_vocab=N_VOCAB, ld=LD):
    """cases -> logits [rows + 1][ld] (guard columns and a guard row of SENTINEL), histories, n_cur, done (the guard row is done), names"""
    names = list(cases)
    rng = np.random.default_rng(seed)
    rows = len(names)
    lg = np.full((rows + 1, ld), SENTINEL, np.float32)
    lg[:rows, :n_vocab] = (rng.standard_normal((rows, n_vocab)) * 3).astype(np.float32)
    hist = np.zeros((rows + 1, MAX_TOKENS), np.int32)
    n_cur = np.zeros(rows + 1, np.int32)
    done = np.ones(rows + 1, np.int32)
    for r, name in enumerate(names):
        hist[r], n_cur[r], done[r], plant = cases[name]
        for c, v in plant.items():
            lg[r, c] = v
    hist[rows] = 20                                           # the guard row's history would match, were it live
    n_cur[rows] = 1
    return lg, hist, n_cur, done, names


def expected(phrases, penalty, lg, hist, n_cur, done, n_vocab=N_VOCAB, eot=EOT, row_mul=1, group=1, fault=None, fn=None):
    """what the launch must leave: (logits, list_logprob [entries] in float64 with SENTINEL where nothing is written).  Launch row r
    changes logits row r with the history of row h = r * row_mul under n_cur / done [h // group]; n_cur None: empty histories.
    fn: a rule with rule()'s signature to use in its place (the CPU test passes the library's host twin)"""
    want = np.array(lg, dtype=np.float32, copy=True)
    lps = np.full(len(done), float(SENTINEL), np.float64)
    for r in range(lg.shape[0]):
        h = r * row_mul
        w = h // group
        if done[w]:
            continue
        n = 0 if n_cur is None else int(n_cur[w])
        row, lp = (fn or rule)(phrases, penalty, hist[h], n, lg[r, :n_vocab], eot, **({"fault": fault} if fault else {}))
        want[r, :n_vocab] = row
        if lp is not None and h % group == 0:
            lps[w] = lp
    return want, lps


def same_words(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def lp_agree(got, want, n_text):
    """list_logprob entries: SENTINEL and -inf exactly, everything else within lp_tol"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    exact = ~np.isfinite(want) | (want == float(SENTINEL))
    with np.errstate(invalid="ignore"):                       # -inf against -inf is settled by the exact comparison
        ok = np.where(exact, got == want, np.abs(got - want) <= lp_tol(n_text))
    return bool(ok.all())


# ---- a Python trie for the builder's test -------------------------------------------------------------------------------------
def trie(phrases):
    """the anchored trie as include/ohw.h lays it out: dict of arrays like CommandTable.arrays()"""
    phrases = [tuple(int(x) for x in p) for p in phrases]
    depth_start, path_base, child_off, path, child_tok, terminal, phrase_id = [], [], [0], [], [], [], []
    for d in range(MAX_LEN + 1):
        depth_start.append(len(terminal))
        path_base.append(len(path))
        for node in sorted({p[:d] for p in phrases if len(p) >= d}):
            path += list(node)
            ids = [i for i, p in enumerate(phrases) if p == node]
            terminal.append(int(bool(ids)))
            phrase_id.append(ids[0] if ids else -1)
            child_tok += sorted({p[d] for p in phrases if len(p) > d and p[:d] == node})
            child_off.append(len(child_tok))
    depth_start.append(len(terminal))
    if not phrases:
        child_off = [0]
    return {"n_phrases": len(phrases), "depth_start": depth_start, "path_base": path_base, "child_off": child_off, "path": path,
            "child_tok": child_tok, "terminal": terminal, "phrase_id": phrase_id}
