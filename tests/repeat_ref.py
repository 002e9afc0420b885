"""Repetition penalty and no-repeat n-grams in numpy: the rule of include/ohw.h (ohw_state_set_repeat_rule), restated from the
definition and not from the library's code, and the cases the CPU and the GPU tests share.

rule(penalty, ngram, history, n_cur, row) -> the row after the rule.  The penalty is float32 arithmetic (x * theta or x / theta,
one rounding), so results are compared as 32-bit words and not within a tolerance.
rule(..., fault=NAME) applies a deliberately wrong rule (FAULTS): the CPU test shows that the comparison the GPU test makes
flags each of them on the shared cases.
"""
import numpy as np

BAN = np.float32(-1.0e30)      # OHW_REPEAT_BAN
MAX_NGRAM = 32
FAULTS = ("per_occurrence", "skips_last_start", "reads_n_cur", "bans_timestamp", "penalises_timestamp", "ban_before_penalty")

N_VOCAB, LD, MAX_TOKENS = 1003, 1024, 448
EOT = 900                      # text tokens are 0 .. 899; 900 .. 1002 stand for the special and timestamp ids
TS, TS2 = 950, 951             # two timestamp ids
SENTINEL = np.float32(-12345.678)     # guard columns and the guard row
ROWS = 5                       # case rows per launch; the guard row makes 6


def rule(penalty, ngram, history, n_cur, row, eot=EOT, fault=None):
    """history: the row's buffer [max_tokens] (entries at and behind n_cur are not the row's history).  Returns a new row."""
    out = np.array(row, dtype=np.float32, copy=True)
    hist = [int(x) for x in history]
    h = hist[:n_cur]
    theta = np.float32(penalty)
    n_vocab = out.size

    def text(t, lax=False):
        return 0 <= t < (n_vocab if lax else min(eot, n_vocab))

    def penalise():
        if theta == np.float32(1.0):
            return
        seen = [t for t in h if text(t, fault == "penalises_timestamp")]
        for t in (seen if fault == "per_occurrence" else sorted(set(seen))):
            x = out[t]
            out[t] = np.float32(x * theta) if x < 0 else np.float32(x / theta)

    def ban():
        n = int(ngram)
        if n < 1 or n_cur < n - 1:
            return
        m = n - 1
        tail = h[n_cur - m:]
        if fault == "reads_n_cur" and m > 0 and n_cur < len(hist):
            tail = hist[n_cur + 1 - m:n_cur + 1]          # the tail takes in tokens[n_cur]
        last = n_cur - n - (1 if fault == "skips_last_start" else 0)
        for i in range(0, last + 1):
            if h[i:i + m] == tail:
                f = h[i + m]
                if text(f, fault == "bans_timestamp"):
                    out[f] = BAN

    if fault == "ban_before_penalty":
        ban(); penalise()
    else:
        penalise(); ban()
    return out


# ---- the shared cases ------------------------------------------------------------------------------------------------------
def _hist(tokens, poison=None):
    """a history buffer: the row's tokens, then poison (tokens that would make or break a match if they were read; one value or a
    list that is repeated) or zeros"""
    h = np.zeros(MAX_TOKENS, np.int32)
    n = len(tokens)
    h[:n] = tokens
    if poison is not None and n < MAX_TOKENS:
        p = np.atleast_1d(np.asarray(poison, np.int32))
        h[n:] = np.resize(p, MAX_TOKENS - n)
    return h, n


def _case(tokens, poison=None, done=0, logits=None):
    """-> (history buffer, n_cur, done, {token: logit} to plant in the row)"""
    return _hist(tokens, poison) + (done, logits or {})


FILLER = list(range(100, 100 + 297))                  # distinct text tokens: no n-gram of them occurs twice
STRETCH = list(range(500, 540))                       # the 40-token stretch of the n = 32 case
SIGNS = {5: 2.5, 6: -2.5, 7: 0.0, 8: -0.0, 9: 1e-38, 10: -1.0e30}    # > 0, < 0, +0.0, -0.0, a value that goes subnormal under 1.3, the ban's own value


def groups():
    """[(group name, penalty, ngram, {case name: case})]: one (penalty, ngram) per launch, so the cases are grouped by setting"""
    g = []
    # the ban alone, n = 3; theta = 1.0: no word but the banned ones may move
    c = {}
    c["empty_history"] = _case([], poison=[5, 5, 5])
    c["n_cur_is_n_minus_2"] = _case([5], poison=[5, 5, 5])                  # no tail yet
    c["n_cur_is_n_minus_1"] = _case([5, 5], poison=[5, 5])                  # a tail, no start: reading tokens[2] would find one
    c["n_cur_is_n_no_match"] = _case([5, 6, 7], poison=[6, 7])              # exactly one start, and it differs
    c["aaa"] = _case([5, 5, 5], poison=6)                                   # exactly one start, i = n_cur - n, overlapping the tail
    c["poison_completes_tail"] = _case([5, 6, 7, 5], poison=6)              # tail [7, 5]; with tokens[4] it would be [5, 6] and ban 7
    c["only_start_is_0"] = _case([20, 21, 22] + FILLER[:295] + [20, 21])    # 300 tokens: positions behind the workgroup's width count
    c["only_start_is_last"] = _case(FILLER[:297] + [30, 30, 30], poison=31)
    c["timestamp_in_tail"] = _case([TS, 7, 8, 40, TS, 7])                   # the tail [TS, 7] matches at 0: 8 is banned
    c["timestamp_follower"] = _case([7, 8, TS, 40, 7, 8])                   # the follower of [7, 8] is a timestamp: not banned
    c["two_followers"] = _case([7, 8, 50, 7, 8, 51, 7, 8])
    c["done_row"] = _case([5, 5, 5], done=1)
    c["n_cur_at_max_tokens"] = _case([60, 61, 62] + [1 + (i % 3 == 0) for i in range(MAX_TOKENS - 5)] + [60, 61])
    g.append(("ban3", 1.0, 3, c))
    c = {}
    c["n1_bans_every_text_token"] = _case([5, TS, 6, 5, TS2, 899], poison=7)
    c["n1_empty"] = _case([], poison=7)
    g.append(("ban1", 1.0, 1, c))
    c = {}
    c["aa_n2"] = _case([5, 5], poison=6)
    c["aaa_n2"] = _case([5, 5, 5], poison=6)
    c["n2_no_tail_needed_yet"] = _case([5], poison=5)                       # n_cur = n - 1: a tail, no start
    g.append(("ban2", 1.0, 2, c))
    c = {}
    c["stretch_repeats"] = _case(STRETCH + STRETCH[:35], poison=STRETCH[35:])          # tail = STRETCH[4:35]: start 4 bans STRETCH[35]
    c["stretch_one_short"] = _case(STRETCH[:31], poison=STRETCH[31:])                  # n_cur = n - 1
    c["stretch_exactly_n"] = _case([70] * 32, poison=71)                               # n_cur = n, the one start overlaps the tail
    c["stretch_breaks"] = _case(STRETCH + [99] + STRETCH[5:35])                        # the tail's oldest token differs from start 4's
    g.append(("ban32", 1.0, 32, c))
    # the penalty alone
    for name, theta in (("pen1.3", 1.3), ("pen0.5", 0.5)):
        c = {}
        c["signs"] = _case(list(SIGNS), logits=SIGNS)
        c["seven_times_once"] = _case([5, 6, 5, 5, 7, 5, 5, 6, 5, 5], logits={5: 3.25, 6: -1.75})
        c["timestamps_not_penalised"] = _case([TS, 5, TS, TS2, 899], logits={TS: 4.0, TS2: -4.0, 899: 1.0})
        c["empty_history"] = _case([], poison=5)
        c["poison_not_penalised"] = _case([5], poison=6, logits={6: 2.0})
        c["long_history"] = _case([FILLER[i % 90] for i in range(300)])     # 90 distinct tokens, each 3 or 4 times, behind the workgroup's width too
        c["done_row"] = _case([5, 6], done=1)
        c["n_cur_at_max_tokens"] = _case([(7 * i) % 200 for i in range(MAX_TOKENS)])
        g.append((name, theta, 0, c))
    # both: the ban comes after the penalty
    c = {}
    c["penalised_and_banned"] = _case([5, 6, 5], logits={6: 2.0, 5: -1.0})  # 6 is penalised and banned; 5 is penalised only
    c["timestamp_follower_and_text"] = _case([TS, 5, TS, 5, 6, TS], logits={TS: 1.0})
    c["aaa"] = _case([5, 5, 5], logits={5: -2.0})
    g.append(("pen1.3_ban2", 1.3, 2, c))
    c = {}
    c["penalised_and_banned_n3"] = _case([5, 6, 7, 5, 6], logits={7: -0.5})
    c["long_history_both"] = _case([FILLER[i % 50] for i in range(300)])
    g.append(("pen0.5_ban3", 0.5, 3, c))
    return g


def chunks(cases):
    names = list(cases)
    return [{n: cases[n] for n in names[i:i + ROWS]} for i in range(0, len(names), ROWS)]


def make_rows(cases, seed):
    """logits [rows + 1][LD] for the cases in order, sentinel-filled guard columns and a guard row -> (logits, histories, n_cur,
    done, names)"""
    names = list(cases)
    rng = np.random.default_rng(seed)
    lg = np.full((len(names) + 1, LD), SENTINEL, np.float32)
    lg[:len(names), :N_VOCAB] = (rng.standard_normal((len(names), N_VOCAB)) * 3.0).astype(np.float32)
    for r, n in enumerate(names):
        for t, v in cases[n][3].items():
            lg[r, t] = np.float32(v)
    hist = np.stack([cases[n][0] for n in names] + [np.full(MAX_TOKENS, 5, np.int32)])
    n_cur = np.asarray([cases[n][1] for n in names] + [MAX_TOKENS], np.int32)
    done = np.asarray([cases[n][2] for n in names] + [1], np.int32)       # the guard row is a done row with a full history: nothing may touch it
    return lg, hist, n_cur, done, names


def expected(penalty, ngram, lg, hist, n_cur, done, fault=None, row_mul=1, group=1):
    """the whole buffer after the rule: launch row r changed over [0, N_VOCAB) with the history of row r * row_mul under entry
    r * row_mul // group (n_cur None: every history is empty), everything else as it was"""
    out = lg.copy()
    for r in range(lg.shape[0]):
        h = r * row_mul
        e = h // group
        if done[e]:
            continue
        out[r, :N_VOCAB] = rule(penalty, ngram, hist[h], 0 if n_cur is None else int(n_cur[e]), lg[r, :N_VOCAB], EOT, fault)
    return out


def same_words(a, b):
    """THE comparison of the kernel test: every word of the buffer, guard columns and rows included"""
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def repeated_ngrams(tokens, n, eot):
    """the n-grams whose last token is a text token and that occur more than once in a row of tokens: what a row decoded under
    no_repeat_ngram_size = n may not hold"""
    seen, twice = set(), []
    for i in range(len(tokens) - n + 1):
        g = tuple(int(t) for t in tokens[i:i + n])
        if g[-1] >= eot:
            continue
        if g in seen:
            twice.append(g)
        seen.add(g)
    return twice
