"""Stitched windows: the Python restatement of the seam, range and clip rules (include/ohw.h) and the case table the CPU and
GPU tests share.

seam() is transformers' _find_longest_common_sequence for two sequences, operation for operation in float64 (test_stitch_cpu
pins it to the installed function); its keyword arguments inject one fault each, which the word comparison must flag on the
table.  The rows of the table carry poison behind n_text: a copy of the partner window's tokens, so a read past the end creates
matches."""
import numpy as np

CHUNK = 480000
STRIDE = 448
SENTINEL = -0x35A1


def plan(n, overlap_ms):
    """(hop, windows, [(start, end)]) of a recording of n samples"""
    hop = CHUNK - overlap_ms * 16
    w = 0 if n == 0 else 1 if n <= CHUNK else -((n - CHUNK) // -hop) + 1
    return hop, w, [(k * hop, min(n, k * hop + CHUNK)) for k in range(w)]


_PAD = 3 * STRIDE + 8


def _row(row, fill):
    """a side as an array that any fault may read past: its own tokens (and poison), then a filler no token equals"""
    out = np.full(_PAD + len(row), fill, dtype=np.int64)
    out[:len(row)] = row
    return out


def seam(left_row, L, right_row, R, min_matches=2, strict=True, eps=True, clip_le=True, clip_re=True, overread=0, round_up=False,
         dtype=np.float64):
    """[shift, matches, left_cut, right_cut, L, R] of one seam; left_row / right_row may hold poison behind L / R, which only a
    fault reads"""
    n_left = L
    L = L + overread                           # fault: the left side is staged one token too long
    left, right = _row(left_row, -1), _row(right_row, -2)
    best, best_i, best_m = dtype(0.0), 0, 0
    idx = (L, L, 0, 0)
    for i in range(1, L + R):
        ls, le = max(0, L - i), (min(L, L + R - i) if clip_le else L)
        rs, re = max(0, i - L), (min(R, i) if clip_re else i)
        m = int(np.sum(left[ls:le] == right[rs:rs + le - ls]))
        score = dtype(m) / dtype(i) + (dtype(i) / dtype(10000.0) if eps else dtype(0.0))
        if m >= min_matches and (score > best if strict else score >= best):
            best, best_i, best_m, idx = score, i, m, (ls, le, rs, re)
    up = 1 if round_up else 0
    return [best_i, best_m, (idx[0] + idx[1] + up) // 2, (idx[2] + idx[3] + up) // 2, n_left, R]


def seams(tok, n_text, **fault):
    """int32 [W - 1][8]: the words of every seam of a table (tok [W][stride] with its counts, or a list of token lists)"""
    if not isinstance(tok, np.ndarray):
        n_text = [len(w) for w in tok]
    out = np.zeros((max(len(n_text) - 1, 0), 8), dtype=np.int32)
    for s in range(len(n_text) - 1):
        out[s] = [s] + seam(tok[s], int(n_text[s]), tok[s + 1], int(n_text[s + 1]), **fault) + [0]
    return out


def merge_pair(a, b):
    """what _find_longest_common_sequence([a, b]) returns, by the seam rule"""
    _, _, lc, rc, _, _ = seam(list(a), len(a), list(b), len(b))
    return list(a[:lc]) + list(b[rc:])


def ranges(seam_words, n_text):
    """the text-token range [first, end) every window keeps"""
    out = []
    for w, n in enumerate(n_text):
        rc = 0 if w == 0 else int(seam_words[w - 1][4])
        lc = int(n) if w + 1 == len(n_text) else int(seam_words[w][3])
        out.append((rc, max(rc, lc)))
    return out


def kept_range(tokens, first, end, eot):
    """a text-token range in the positions of a window's kept tokens: an uncut end keeps its timestamp tokens"""
    pos = [i for i, t in enumerate(tokens) if t < eot]
    a = 0 if first == 0 else len(tokens) if first >= len(pos) else pos[first]
    b = len(tokens) if end >= len(pos) else pos[end]
    return a, max(a, b)


def stitch(windows, eot):
    """the windows' kept tokens -> (seam words, [(first, end)] in kept positions, the merged tokens)"""
    text = [[t for t in w if t < eot] for w in windows]
    sw = seams(text, None)
    rg = [kept_range(w, a, b, eot) for w, (a, b) in zip(windows, ranges(sw, [len(t) for t in text]))]
    return sw, rg, [t for w, (a, b) in zip(windows, rg) for t in w[a:b]]


def clip_segment(seg, first, end, t_left, t_right):
    """a segment (first, end, t0, t1) of a window against the range: None when wholly outside"""
    f, e, t0, t1 = seg
    if e <= first or f >= end:
        return None
    clamp = lambda t: min(max(np.float32(t), np.float32(t0)), np.float32(t1))
    if f < first:
        f, t0n = first, clamp(t_left)
    else:
        t0n = np.float32(t0)
    if e > end:
        e, t1n = end, clamp(t_right)
    else:
        t1n = np.float32(t1)
    return (f, e, float(t0n), float(t1n))


def seam_time(w, hop, n):
    """the middle of the audio windows w and w + 1 share, seconds on the recording's clock"""
    return (((w + 1) * hop) / 16000.0 + min(n, w * hop + CHUNK) / 16000.0) / 2.0


# ---- the case table ----------------------------------------------------------------------------------------------------------
def _distinct(rng, n, base):
    return [base + int(x) for x in rng.permutation(20000)[:n]]


def _planted(L, R, plants, base=0):
    """all-distinct sides with matches planted: plants = {shift: count}.  A pair (left a, right b) matches at shift L - a + b only"""
    left, right = [base + 100000 + j for j in range(L)], [base + 200000 + j for j in range(R)]
    used = set()
    for i, m in plants.items():
        ls, le, rs = max(0, L - i), min(L, L + R - i), max(0, i - L)
        js = [j for j in range(le - ls) if rs + j not in used]
        step = max(1, len(js) // m)
        for j in js[::step][:m]:
            right[rs + j] = left[ls + j]
            used.add(rs + j)
    return left, right


def cases():
    """[(name, left, right)]"""
    rng = np.random.default_rng(20240917)
    out = []

    def overlap(name, L, R, k, mismatches=0):
        left = _distinct(rng, L, 0)
        right = left[L - k:] + _distinct(rng, R - k, 20000)
        for x in range(mismatches):
            right[1 + x * max(1, (k - 2) // max(1, mismatches))] = 40000 + x
        out.append((name, left, right[:R]))

    for total in (63, 64, 65, 255, 256, 257):                   # L + R - 1: the last shift at the edges of a wave and of the block
        L = (total + 1) // 2
        overlap("shifts%d" % total, L, total + 1 - L, min(9, L - 1))
    overlap("shifts895", 448, 448, 37)
    out.append(("L0", [], _distinct(rng, 40, 0)))
    out.append(("R0", _distinct(rng, 40, 0), []))
    out.append(("L0R0", [], []))
    out.append(("L1", [7], [7, 7, 8]))
    out.append(("R1", [5, 6, 7], [7]))
    out.append(("L1R1", [7], [7]))
    overlap("L>>R", 400, 12, 8)
    overlap("R>>L", 12, 400, 8)
    big = _distinct(rng, 300, 0)
    out.append(("R inside L", big, big[100:120]))               # the best shift lies past R: re is clipped
    out.append(("L inside R", big[150:170], big))               # and past L
    overlap("planted k=20, 1 mismatch", 150, 170, 20, 1)
    overlap("planted k=31, 2 mismatches", 211, 97, 31, 2)
    out.append(("tie 100/200",) + _planted(300, 300, {100: 2, 200: 2}))           # both score 0.03: the first wins
    out.append(("tie 50/400",) + _planted(300, 300, {50: 2, 400: 2}))             # 400 is thread 143's second shift, 50 is thread 49's first
    out.append(("tie 125/160",) + _planted(300, 300, {125: 2, 160: 2}))
    out.append(("tie 125/160 under a later best",) + _planted(300, 300, {160: 2, 125: 2, 300: 2}))
    out.append(("one match only",) + _planted(120, 90, {30: 1, 77: 1, 150: 1}))   # unmatched
    out.append(("no match", _distinct(rng, 50, 0), _distinct(rng, 60, 20000)))
    per = [11, 12, 13] * 40
    out.append(("period 3", per[:100], per[1:91]))                                # many shifts of ratio 1: the eps term decides
    out.append(("period 3 aligned", per[:90], per[:60]))
    # float64 keeps shift 200 (16 / 200 + 0.02 = 0.1 above 9 / 100 + 0.01 = 0.09999999999999999); in fp32 shift 100 scores higher
    out.append(("fp32 picks another shift",) + _planted(300, 300, {100: 9, 200: 16}))
    out.append(("odd midpoint", [1, 2, 3, 4, 5, 6, 7], [5, 6, 7, 9]))
    while len(out) < 150:
        L, R = int(rng.integers(0, 120)), int(rng.integers(0, 120))
        k = int(rng.integers(0, min(L, R) + 1))
        if rng.random() < 0.3:
            out.append(("random %d" % len(out), [int(x) for x in rng.integers(0, 6, L)], [int(x) for x in rng.integers(0, 6, R)]))
        else:
            overlap("random overlap %d" % len(out), L, R, k, int(rng.integers(0, 3)) if k > 6 else 0)
    return out


_TABLE = None


def table():
    """(tok int32 [300][448], n_text int32 [300], names): case k is windows 2k (left) and 2k + 1 (right); the seams between two
    cases are cases too.  Behind n_text every row holds its partner's tokens, cyclically, the left rows from the token behind the
    partner's best overlap on"""
    global _TABLE
    if _TABLE is None:
        cs = cases()
        tok = np.zeros((2 * len(cs), STRIDE), dtype=np.int32)
        n_text = np.zeros(2 * len(cs), dtype=np.int32)
        for k, (_, left, right) in enumerate(cs):
            shift = seam(left, len(left), right, len(right))[0]
            for w, own, other, start in ((2 * k, left, right, min(shift, len(left))), (2 * k + 1, right, left, 0)):
                n_text[w] = len(own)
                tok[w, :len(own)] = own
                fill = [other[(start + j) % len(other)] for j in range(STRIDE - len(own))] if other else [own[0] if own else 1] * (STRIDE - len(own))
                tok[w, len(own):] = fill
        tok.setflags(write=False)
        n_text.setflags(write=False)
        _TABLE = (tok, n_text, [c[0] for c in cs], seams(tok, n_text))
        _TABLE[3].setflags(write=False)
    return _TABLE
