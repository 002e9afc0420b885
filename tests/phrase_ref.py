"""Hot phrases in numpy: the builder and the rule of include/ohw.h (ohw_state_set_phrase_table), restated from the
definition and not from the library's code, and the cases the CPU and the GPU tests share.

build(phrases, boosts) -> the flat trie as a dict of arrays (the layout of ohw_phrase_table);
boost(table, history, n_cur, row) -> the row after the rule: float32 adds in table order (depth ascending, children by token).
boost(..., fault=NAME) applies a deliberately wrong rule (FAULTS): the CPU test shows that the comparison the GPU test makes
flags each of them on the shared cases.
"""
import numpy as np

MAX_LEN, MAX_PHRASES = 16, 1024
FAULTS = ("tail_off_by_one", "reads_n_cur", "drops_last_child", "deepest_only")

N_VOCAB, LD, MAX_TOKENS = 1003, 1024, 24
EOT = 900                      # text tokens are 0 .. 899; 900 .. 1002 stand for the special and timestamp ids
TS = 950                       # a timestamp id
# a node with 1024 children needs 1024 text tokens, more than a vocabulary of 1003 holds: that one table runs at the smallest
# odd size with room for them (children 30 .. 1053)
WIDE_VOCAB, WIDE_LD, WIDE_EOT = 1091, 1120, 1060
SENTINEL = np.float32(-12345.678)     # guard columns and the guard row


def build(phrases, boosts):
    """the trie: only prefixes with a continuation are nodes; nodes by depth, then by path; an edge's boost is the maximum over
    the phrases through it (the first one seen stays on a tie)"""
    nodes = {}                                   # (depth, path) -> {token: boost}
    for p, b in zip(phrases, boosts):
        p = [int(t) for t in p]
        for d in range(len(p)):
            ch = nodes.setdefault((d, tuple(p[:d])), {})
            if p[d] not in ch or np.float32(b) > ch[p[d]]:
                ch[p[d]] = np.float32(b)
    order = sorted(nodes)                        # tuples compare lexicographically
    depth_start = np.zeros(MAX_LEN + 1, np.int32)
    path_base = np.zeros(MAX_LEN, np.int32)
    child_off, path, child_tok, child_boost = [0], [], [], []
    for d in range(MAX_LEN):
        depth_start[d] = len(child_off) - 1
        path_base[d] = len(path)
        for key in order:
            if key[0] != d:
                continue
            path.extend(key[1])
            for t in sorted(nodes[key]):
                child_tok.append(t)
                child_boost.append(nodes[key][t])
            child_off.append(len(child_tok))
    depth_start[MAX_LEN] = len(child_off) - 1
    return {"n_phrases": len(phrases), "depth_start": depth_start, "path_base": path_base, "child_off": np.asarray(child_off, np.int32),
            "path": np.asarray(path, np.int32), "child_tok": np.asarray(child_tok, np.int32), "child_boost": np.asarray(child_boost, np.float32)}


def node_path(t, n, d):
    o = int(t["path_base"][d]) + (n - int(t["depth_start"][d])) * d
    return [int(x) for x in t["path"][o:o + d]]


def boost(t, history, n_cur, row, fault=None):
    """history: the row's buffer [max_tokens] (entries at and behind n_cur are not the row's history).  Returns a new row."""
    out = np.array(row, dtype=np.float32, copy=True)
    hist = [int(x) for x in history]
    matches = []
    for d in range(MAX_LEN):
        end = n_cur
        if fault == "tail_off_by_one" and d > 0:
            end = n_cur - 1                      # the window ends one token early
        if fault == "reads_n_cur" and d > 0 and n_cur < len(hist):
            end = n_cur + 1                      # the window takes in tokens[n_cur]
        if d > end:
            break
        tail = hist[end - d:end]
        for n in range(int(t["depth_start"][d]), int(t["depth_start"][d + 1])):
            if node_path(t, n, d) == tail:
                matches.append(n)
                break
    if fault == "deepest_only":
        matches = matches[-1:]
    for n in matches:
        e0, e1 = int(t["child_off"][n]), int(t["child_off"][n + 1])
        if fault == "drops_last_child" and e1 - e0 > 1:
            e1 -= 1
        for e in range(e0, e1):
            k = int(t["child_tok"][e])
            out[k] = np.float32(out[k] + t["child_boost"][e])
    return out


def tables_equal(a, b):
    """a, b: dicts as build() returns (the library's table through PhraseTable.arrays()); boosts compared as words"""
    if int(a["n_phrases"]) != int(b["n_phrases"]):
        return False
    for k in ("depth_start", "path_base", "child_off", "path", "child_tok"):
        if not np.array_equal(np.asarray(a[k], np.int32), np.asarray(b[k], np.int32)):
            return False
    return np.array_equal(np.asarray(a["child_boost"], np.float32).view(np.uint32), np.asarray(b["child_boost"], np.float32).view(np.uint32))


# ---- the shared cases ------------------------------------------------------------------------------------------------------
DEEP = list(range(100, 116))                          # a 16-token phrase: nodes of every depth 0 .. 15
WIDE = [[7, 30 + i] for i in range(1024)]             # the node behind token 7 has 1024 children


def base_table():
    """phrases that make every listed case possible -> (phrases, boosts)"""
    phrases = [[10, 11, 12], [11, 12], [10, 11, 13], [20], [30, 31], DEEP, [12, 40], [10, 11, 12, 50]]
    boosts = [1.5, 2.25, 0.75, 3.0, -1.25, 0.5, 4.0, 1e-3]
    return phrases, boosts


def wide_table():
    """1024 phrases, the limit, all behind token 7 -> (phrases, boosts); tokens below WIDE_EOT"""
    return WIDE, [0.001 * (i + 1) for i in range(1024)]


def _hist(tokens, poison=None):
    """a history buffer: the row's tokens, then poison (tokens that would complete a match if they were read) or zeros"""
    h = np.zeros(MAX_TOKENS, np.int32)
    h[:len(tokens)] = tokens
    if poison is not None:
        h[len(tokens):] = poison
    return h, len(tokens)


def base_cases():
    """name -> (history buffer, n_cur, done) under base_table().  Poisoned buffers hold, at and behind n_cur, a token that
    would extend the tail into a deeper match"""
    c = {}
    c["empty_history"] = _hist([]) + (0,)
    c["empty_history_poison"] = _hist([], poison=10) + (0,)                    # reading tokens[0] would match the node [10]
    c["depth1"] = _hist([5, 30]) + (0,)
    c["depth15"] = _hist([3] + DEEP[:15]) + (0,)
    c["depth15_exact_length"] = _hist(DEEP[:15]) + (0,)
    c["shorter_than_depth"] = _hist([11]) + (0,)                               # the node [10, 11] needs two tokens
    c["oldest_differs"] = _hist([99] + DEEP[1:15]) + (0,)                      # equals the depth-15 path but for its oldest token
    c["timestamp_in_tail"] = _hist([10, TS, 11]) + (0,)
    c["timestamp_last"] = _hist([10, 11, TS]) + (0,)
    c["nested"] = _hist([10, 11]) + (0,)                                       # [10, 11] and [11] both raise 12; the root too
    c["nested_deeper"] = _hist([4, 10, 11, 12]) + (0,)
    c["poison_extends"] = _hist([10], poison=11) + (0,)                        # tokens[n_cur] = 11 would make the tail [10, 11]
    c["poison_after_two"] = _hist([10, 11], poison=12) + (0,)
    c["done_row"] = _hist([10, 11]) + (1,)
    full = [1] * (MAX_TOKENS - 2) + [10, 11]
    c["n_cur_at_max_tokens"] = _hist(full) + (0,)
    return c


def wide_cases():
    c = {}
    c["wide_node"] = _hist([2, 7]) + (0,)
    c["wide_root_only"] = _hist([2, 30]) + (0,)
    c["wide_poison"] = _hist([2], poison=7) + (0,)
    return c


def make_rows(cases, seed, n_vocab=N_VOCAB, ld=LD):
    """logits [rows + 1][ld] for the cases in order, sentinel-filled guard columns and a guard row -> (logits, histories, n_cur,
    done, names)"""
    names = list(cases)
    rng = np.random.default_rng(seed)
    lg = np.full((len(names) + 1, ld), SENTINEL, np.float32)
    lg[:len(names), :n_vocab] = (rng.standard_normal((len(names), n_vocab)) * 3.0).astype(np.float32)
    hist = np.stack([cases[n][0] for n in names] + [np.zeros(MAX_TOKENS, np.int32)])
    n_cur = np.asarray([cases[n][1] for n in names] + [0], np.int32)
    done = np.asarray([cases[n][2] for n in names] + [1], np.int32)       # the guard row is a done row: nothing may touch it
    return lg, hist, n_cur, done, names


def expected(table, lg, hist, n_cur, done, fault=None, n_vocab=N_VOCAB):
    """the whole buffer after the rule: live rows boosted over [0, n_vocab), everything else as it was"""
    out = lg.copy()
    for r in range(lg.shape[0]):
        if done[r]:
            continue
        out[r, :n_vocab] = boost(table, hist[r], int(n_cur[r]), lg[r, :n_vocab], fault)
    return out


def same_words(a, b):
    """THE comparison of the kernel test: every word of the buffer, guard columns and rows included"""
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))
