"""Needle inputs for the attention kernels, and their float64 reference.

The synthetic models of the suite have diffuse attention (weights are zero-mean with variance 1 / fan_in, so no key gets more
than about 1 % of a softmax over 1500 keys): a kernel that drops, adds or misplaces ONE key moves its output by less than any
end-to-end tolerance.  Here every query is built so that one key (or an exactly known pair) decides its output:

  keys     K[j]  random +-1 vectors of 64 entries, one per (slab, head, position)
  values   V[j]  multiples of 2^-6 in [-1, 1)
  queries  G * K[needle]: the scaled score q.k / 8 is 8 G on the needle and G * dot / 8 (|dot| about 40 at most) elsewhere
  poison   every key a query must NOT see (past a window's length, past the causal limit, in a cache row the slot table does not
           name) is 2 * K[needle of some query that could reach it by mistake] with the value row 100.0: it would outscore the
           needle.  Finite on purpose: a kernel may load a dead row and multiply it by p = 0.

Everything is exactly representable in bf16 and f16.  Patterns: "sharp" (G = 8, needle weight 1 - 1e-11), "pair" (the query is
G / 2 * (K[a] + K[b]) with a and b in different key blocks / slices / chunks, so the output is (V[a] + V[b]) / 2 and has to
survive the rescale and the merge of partial states), "soft" (G = 2: needle weight >= 0.997 and a real diffuse remainder).

A Case names, for every query row, the positions it may see (always 0 .. n_keys - 1) and the slab (window / cache row) that
holds each of them; reference() is a softmax over exactly those keys, written from the definition.  The fault-injection tests
(test_attn_needles_cpu.py) edit that description, never a kernel.
"""
import numpy as np

DH = 64
SENTINEL = 77.0          # what the GPU tests pre-fill outputs with (exact in bf16 / f16)
POISON_V = 100.0
PATTERNS = ("sharp", "pair", "soft")
GAIN = {"sharp": 8.0, "pair": 8.0, "soft": 2.0}
# |out - reference| <= TOL[dtype] * max|V|, max|V| = 1.  Half an ulp of the output rounding is 2^-9 (bf16) / 2^-12 (f16) at
# |out| < 1; the encoder kernel rounds P to 16 bits before P.V, at most as much again since sum p |v| <= 1; fp32 accumulation
# noise is negligible; the sum is doubled for margin.
TOL = {0: 2.0 ** -7, 1: 2.0 ** -10}
# needle weights the construction guarantees (float64 softmax; asserted for every case by test_attn_needles_cpu.py)
# pair: a and b always tie (q . K[a] == q . K[b]); where the partner is forced (one key in the other block) a third key may
# come close, and 1e-3 of stray weight moves the output by 1e-3 at most - the reference carries it exactly either way
MIN_WEIGHT = {"sharp": 1.0 - 1e-11, "pair": 0.999, "soft": 0.997}

XA_MAX_SPLIT = 8


class Case:
    """q [R][H][64]; K, V [S][H][P][64] (the memory image, poison included); n_keys [R]; slab [R][P]: the slab that holds
    position j of row r's sequence; needle / needle2 [R][H]: positions a and b (b == a outside the pair pattern);
    units: list of [P] arrays - the kernel's partition(s) of the positions, first the one a pair must straddle"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def R(self):
        return self.q.shape[0]

    @property
    def H(self):
        return self.q.shape[1]


def reference(c, edit=None, slab=None, head_map=None, scale=None, weights=False):
    """softmax(q . K^T / 8) V over exactly the allowed keys of every row, float64 -> [R][H * 64] row-major.
    The remaining arguments inject faults: edit(r, pos) -> pos changes the positions row r sees, slab replaces the slab table,
    head_map[h] the head whose K / V head h reads, scale(r, h, pos, p) -> p reweights the unnormalised probabilities.
    weights = True also returns [R][H]: the weight on the keys equal to the needle key(s)"""
    slab = c.slab if slab is None else slab
    out = np.zeros((c.R, c.H * DH))
    wts = np.zeros((c.R, c.H))
    for r in range(c.R):
        pos = np.arange(int(c.n_keys[r]))
        if edit is not None:
            pos = np.asarray(edit(r, pos), dtype=np.int64)
        s = slab[r, pos]
        for h in range(c.H):
            hk = h if head_map is None else head_map[h]
            if edit is None and (s == s[0]).all():
                k, v = c.K[s[0], hk, :len(pos)], c.V[s[0], hk, :len(pos)]      # a view: the common case, no gather
            else:
                k, v = c.K[s, hk, pos], c.V[s, hk, pos]
            sc = k @ c.q[r, h] / 8.0
            p = np.exp(sc - sc.max())
            if scale is not None:
                p = scale(r, h, pos, p)
            p = p / p.sum()
            out[r, h * DH:(h + 1) * DH] = p @ v
            if weights:
                ka, kb = c.K[slab[r, c.needle[r, h]], hk, c.needle[r, h]], c.K[slab[r, c.needle2[r, h]], hk, c.needle2[r, h]]
                wts[r, h] = p[(k == ka).all(axis=1) | (k == kb).all(axis=1)].sum()
    return (out, wts) if weights else out


def worst_error(got, want):
    """the comparison of the GPU tests: the largest absolute difference (max|V| = 1, so TOL is absolute)"""
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max())


def act_tiled_index(M, d):
    """act_tiled_offset (common.hpp) as an index array [M][d]: element (m, k) of an activation-tile buffer
    [ceil(M / 16)][d / 32][64][8] lies at ((((m / 16) * (d / 32) + k / 32) * 64 + m % 16 + 16 * ((k % 32) / 8)) * 8) + k % 8"""
    m = np.arange(M, dtype=np.int64)[:, None]
    k = np.arange(d, dtype=np.int64)[None, :]
    return ((((m >> 4) * (d >> 5) + (k >> 5)) * 64 + (m & 15) + 16 * ((k & 31) >> 3)) << 3) + (k & 7)


def tiled_elems(M, d):
    return (M + 15) // 16 * 16 * d


# ---- construction ------------------------------------------------------------------------------------------------------

def _keys(rng, shape):
    return rng.integers(0, 2, size=shape + (DH,)).astype(np.float64) * 2.0 - 1.0


def _values(rng, shape):
    return rng.integers(-64, 64, size=shape + (DH,)).astype(np.float64) / 64.0


def xattn_split(M, n_head, t_len):
    """launch_cross_attn's number of key slices when a split form may be picked"""
    ks = 1
    while ks < XA_MAX_SPLIT and M * n_head * ks < 512 and t_len // (ks * 2) >= 64:
        ks *= 2
    return ks


def xattn_slice_of(t, ks):
    """cross_attn_kernel's slice rule: ceil(ceil(t / 8) / ks) groups of 8 keys per slice -> slice of every position [t]"""
    per_slice = -(-(-(-t // 8)) // ks)
    return np.arange(t) // 8 // per_slice


def _edges(n, units):
    """positions where kernels go wrong: first and last key, and both sides of every boundary of the primary unit"""
    e = {0, n - 1}
    u = units[0][:n]
    for j in np.nonzero(u[1:] != u[:-1])[0]:
        e.update((int(j), int(j) + 1))
    return sorted(e)


def _second(rng, c_units, n, a):
    """a partner for needle a among positions 0 .. n - 1: in another unit of every partition that has more than one, relaxing
    the later partitions first when nothing is left"""
    if n == 1:
        return a
    for depth in range(len(c_units), -1, -1):
        ok = np.ones(n, dtype=bool)
        ok[a] = False
        for u in c_units[:depth]:
            if len(np.unique(u[:n])) > 1:
                ok &= u[:n] != u[a]
        cand = np.nonzero(ok)[0]
        if len(cand):
            return int(rng.choice(cand))
    return a


def _finish(rng, c, pattern, redraw=True):
    """queries from the final K: G * K[a], or G / 2 * (K[a] + K[b]).  A draw whose needle weight misses MIN_WEIGHT (a key that
    happens to lie close to the needle) is drawn again: b of a pair, and with redraw the needle a itself (at random)"""
    g = GAIN[pattern]
    c.gain, c.pattern = g, pattern
    c.needle2 = c.needle.copy()
    c.q = np.zeros((len(c.n_keys), c.K.shape[1], DH))
    for r in range(c.R):
        n = int(c.n_keys[r])
        s = c.slab[r, :n]
        for h in range(c.H):
            k = c.K[s[0], h, :n] if (s == s[0]).all() else c.K[s, h, np.arange(n)]
            a = int(c.needle[r, h])
            for _ in range(64):
                b = _second(rng, c.units, n, a) if pattern == "pair" else a
                q = g / 2 * (k[a] + k[b])
                sc = k @ q / 8.0
                p = np.exp(sc - sc.max())
                if p[(k == k[a]).all(axis=1) | (k == k[b]).all(axis=1)].sum() >= MIN_WEIGHT[pattern] * p.sum():
                    break
                if redraw and pattern != "pair":
                    a = int(rng.integers(0, n))
            c.needle[r, h], c.needle2[r, h], c.q[r, h] = a, b, q
    return c


def _assign(rng, n_rows, n, edges, start):
    """needles of n_rows queries that all see positions 0 .. n - 1: the edges first (on random rows, from edge `start` on so
    that windows of one row each still walk through all of them), the rest random"""
    pi = rng.integers(0, n, size=n_rows)
    rows = rng.permutation(n_rows)
    for i in range(min(n_rows, len(edges))):
        pi[rows[i]] = edges[(start + i) % len(edges)]
    return pi


def windows_case(seed, pattern, lens, P, rows_of, units_of, H=2):
    """encoder and cross-attention: S = len(lens) windows with P positions in memory each, window w's first lens[w] are its
    keys, the rest poison.  rows_of[w]: the query rows of window w; units_of(n) -> partitions of n keys"""
    rng = np.random.default_rng(seed)
    S = len(lens)
    R = sum(len(x) for x in rows_of)
    c = Case(K=_keys(rng, (S, H, P)), V=_values(rng, (S, H, P)), n_keys=np.zeros(R, dtype=np.int64),
             slab=np.zeros((R, P), dtype=np.int64), needle=np.zeros((R, H), dtype=np.int64), window=np.zeros(R, dtype=np.int64),
             lens=list(lens), units=units_of(P))
    start = int(rng.integers(0, 1 << 20))
    for w, rows in enumerate(rows_of):
        rows = np.asarray(rows, dtype=np.int64)
        n = int(lens[w])
        c.n_keys[rows], c.slab[rows], c.window[rows] = n, w, w
        wu = units_of(n)
        for h in range(H):
            c.needle[rows, h] = _assign(rng, len(rows), n, _edges(n, wu), start)
            start += len(rows)
    _finish(rng, c, pattern)
    for w, rows in enumerate(rows_of):
        n = int(lens[w])
        for h in range(H):
            # dead positions: the first one belongs to this window's first row, and so on round the rows
            for j in range(n, P):
                c.K[w, h, j] = 2.0 * c.K[w, h, c.needle[rows[(j - n) % len(rows)], h]]
                c.V[w, h, j] = POISON_V
    return c


def encoder_case(seed, pattern, B, T, H, lens=None):
    """B windows of T rows, H heads; lens: per-window lengths (VAR / PACKED), else all T.  Query rows are (window, position) for
    the positions inside the window's length, in window order; c.row_pos[r] is the position"""
    lens = [T] * B if lens is None else list(lens)
    rows_of, row_pos, r = [], [], 0
    for n in lens:
        rows_of.append(list(range(r, r + n)))
        row_pos += list(range(n))
        r += n
    c = windows_case(seed, pattern, lens, T, rows_of, lambda n: [np.arange(n) // 64], H=H)
    c.row_pos = np.asarray(row_pos)
    c.T = T
    return c


def encoder_qkv(c, packed=False, guard=0):
    """the encoder kernel's input image [rows][3 * d] (q | k | v, head h at columns h * 64) and, per query row of the case, its
    row in that image.  Unpacked: window b at row b * T, the rows past a window's length carry poison keys / values and a
    needle-strength query; packed: the windows end to end, then `guard` poison rows"""
    S, H, T = c.K.shape[0], c.H, c.T
    d = H * DH
    starts = np.concatenate([[0], np.cumsum(c.lens)])[:-1] if packed else np.arange(S) * T
    n_rows = (int(np.sum(c.lens)) + guard) if packed else S * T
    img = np.zeros((n_rows, 3, H, DH))
    img[:, 0] = 8.0                 # queries of rows no window owns: any finite value
    img[:, 1] = 2.0
    img[:, 2] = POISON_V
    for w in range(S):
        n = c.lens[w] if packed else T
        img[starts[w]:starts[w] + n, 1] = c.K[w, :, :n].transpose(1, 0, 2)
        img[starts[w]:starts[w] + n, 2] = c.V[w, :, :n].transpose(1, 0, 2)
    where = starts[c.window] + c.row_pos
    img[where, 0] = c.q
    if packed:                      # the guard rows sit just behind the last window's keys: its queries' needles, doubled
        last = np.nonzero(c.window == S - 1)[0]
        for g in range(guard):
            r = last[g % len(last)]
            img[n_rows - guard + g, 1] = 2.0 * c.K[S - 1, np.arange(H), c.needle[r]]
    return img.reshape(n_rows, 3 * d), where


def cross_case(seed, pattern, M, n_new, t_len, kv_group=1, lens=None, ks=1, H=2):
    """cross-attention: row m reads window m / n_new (m / kv_group for beams); ks: the key slices the launch is expected to use"""
    per = kv_group if kv_group > 1 else n_new
    W = M // per
    lens = [t_len] * W if lens is None else list(lens)
    rows_of = [list(range(w * per, (w + 1) * per)) for w in range(W)]

    def units_of(n):
        pos = np.arange(n)
        return [xattn_slice_of(n, ks), pos // 8 % 4, pos % 8]
    c = windows_case(seed, pattern, lens, t_len, rows_of, units_of, H=H)
    c.ks = ks
    return c


def self_case(seed, pattern, n_past, n_new, n_ctx, slots=False, H=2):
    """masked self-attention: W = len(n_past) windows / cache rows, new token i of window b sees positions 0 .. n_past[b] + i.
    Plain: position j of window b lives in cache row b.  slots: in row slot[b][j] of a random table; the same position of every
    row that no window names is poison.  The position just past query i's limit is still inside the window for i < n_new - 1
    (it is new token i + 1's key): it holds a copy of K[needle(i)] with a value row of its own - a twin that ties with the
    needle if query i reads it and is an ordinary key for the later queries.  Positions past the window are plain poison"""
    rng = np.random.default_rng(seed)
    W = len(n_past)
    R = W * n_new
    n_past = np.asarray(n_past, dtype=np.int64)
    table = rng.integers(0, W, size=(W, n_ctx)) if slots else np.repeat(np.arange(W)[:, None], n_ctx, axis=1)
    c = Case(K=_keys(rng, (W, H, n_ctx)), V=_values(rng, (W, H, n_ctx)), n_keys=np.zeros(R, dtype=np.int64),
             slab=np.repeat(table, n_new, axis=0), needle=np.zeros((R, H), dtype=np.int64), window=np.repeat(np.arange(W), n_new),
             units=[np.arange(n_ctx) // 64], n_past=n_past, n_new=n_new, table=table if slots else None)
    live = np.zeros((W, n_ctx), dtype=bool)              # cells (cache row, position) some window's sequence names
    for b in range(W):
        j = np.arange(n_past[b] + n_new)
        live[table[b, j], j] = True
    for b in range(W):
        for i in range(n_new):
            r = b * n_new + i
            n = int(n_past[b]) + i + 1
            c.n_keys[r] = n
            for h in range(H):
                # the last allowed key half of the time for the new tokens after the first, else one of the edges or any key
                edges = _edges(n, c.units)
                u = rng.random()
                a = n - 1 if (i > 0 and u < 0.5) else int(rng.choice(edges)) if u < 0.8 else int(rng.integers(0, n))
                c.needle[r, h] = a
                if i < n_new - 1:
                    c.K[table[b, n], h, n] = c.K[table[b, a], h, a]
    for s in range(W):
        for j in range(n_ctx):
            if live[s, j]:
                continue
            # whose needle the dead cell doubles.  Plain: only window s reads row s - its last query for the first dead
            # position, then round its queries.  slots: a window whose limit the cell sits just behind, else one that reads
            # position j from another row, else any; that window's last query sees the most keys
            if not slots:
                b = s
                r = b * n_new + (n_new - 1 - (j - int(n_past[b]) - n_new)) % n_new
            else:
                first = [b for b in range(W) if table[b, j] == s and j == n_past[b] + n_new]
                reach = [b for b in range(W) if j < n_past[b] + n_new]
                b = first[0] if first else reach[(s + j) % len(reach)] if reach else (s + j) % W
                r = b * n_new + n_new - 1
            for h in range(H):
                a = c.needle[r, h]
                c.K[s, h, j] = 2.0 * c.K[table[b, a], h, a]
            c.V[s, :, j] = POISON_V
    return _finish(rng, c, pattern, redraw=False)      # the twins are copies of the needles drawn above


# ---- the cases of tests/test_gpu_attn_needles.py (test_attn_needles_cpu.py checks the construction at every one) ---------
VAR_LENS = [300, 1, 129, 64, 65]          # envelope 300: query blocks wholly past a length, ragged and whole key blocks
XA_LENS = [250, 1, 63, 8]                 # envelope 250

# name -> (B, T, H, lens, mode); 128 query rows per workgroup: the workgroup count is ceil(T / 128) * H * B
ENCODER_CASES = {f"T{T}": (2, T, 2, None, "uniform") for T in (1, 31, 64, 65, 128, 129, 191, 300)}
ENCODER_CASES.update({
    "T1500": (1, 1500, 2, None, "uniform"),        # 24 key blocks, a tail of 28
    "wg6": (1, 300, 2, None, "uniform"),           # 6, 9 and 17 workgroups: xcd_remap's remainder branch
    "wg9": (1, 300, 3, None, "uniform"),
    "wg17": (17, 65, 1, None, "uniform"),
    "var": (5, 300, 2, VAR_LENS, "var"),
    "packed": (5, 300, 2, VAR_LENS, "packed"),
})

# name -> dict(M, n_new, t_len, kv_group, invariant, scratch, lens, done, variant); scratch: partials / tickets are passed
def _xa(M, t_len, variant, n_new=1, kv_group=1, invariant=False, scratch=True, lens=None, done=None):
    return dict(M=M, n_new=n_new, t_len=t_len, kv_group=kv_group, invariant=invariant, scratch=scratch, lens=lens, done=done, variant=variant)


CROSS_CASES = {}
for _t in (5, 8, 63):
    for _m in (1, 3, 17):
        CROSS_CASES[f"plain_t{_t}_m{_m}"] = _xa(_m, _t, "plain")
for _t in (250, 1500):                    # 250: a 2-way split; 1500: 8 slices, the last one short, the last group of 4 keys
    for _m in (1, 3, 17):
        CROSS_CASES[f"split_t{_t}_m{_m}"] = _xa(_m, _t, "split")
    CROSS_CASES[f"plain_t{_t}_invariant"] = _xa(3, _t, "plain", invariant=True)
    CROSS_CASES[f"plain_t{_t}_noscratch"] = _xa(17, _t, "plain", scratch=False)
CROSS_CASES.update({
    "rows2_t5": _xa(2, 5, "rows2", n_new=2, invariant=True),
    "rows2_t250": _xa(6, 250, "rows2", n_new=2, invariant=True),
    "rows3_t8": _xa(3, 8, "rows3", n_new=3, invariant=True),
    "rows3_t1500": _xa(3, 1500, "rows3", n_new=3, invariant=True),
    "rows4_t63": _xa(20, 63, "rows4", n_new=4, invariant=True),
    "rows4_t1500": _xa(4, 1500, "rows4", n_new=4, invariant=True),
    "group2_t1500": _xa(4, 1500, "group2", kv_group=2, invariant=True),
    "group3_t250": _xa(6, 250, "group3", kv_group=3, invariant=True),
    "group4_t63": _xa(8, 63, "group4", kv_group=4, scratch=False),
    "group5_t8": _xa(10, 8, "group5", kv_group=5, invariant=True),
    "group5_t1500": _xa(10, 1500, "group5", kv_group=5, invariant=True),
    "group_split_t63": _xa(4, 63, "group_split", kv_group=2),
    "group_split_t250": _xa(10, 250, "group_split", kv_group=5),
    "group_split_t1500": _xa(6, 1500, "group_split", kv_group=3),
    "var_plain": _xa(4, 250, "plain", lens=XA_LENS),
    "var_rows2": _xa(8, 250, "rows2", n_new=2, lens=XA_LENS),
    "var_rows3": _xa(12, 250, "rows3", n_new=3, lens=XA_LENS),
    "var_rows4": _xa(16, 250, "rows4", n_new=4, lens=XA_LENS),
    "done_plain": _xa(3, 63, "plain", done=[0, 1, 0]),
    "done_split": _xa(3, 1500, "split", done=[1, 0, 0]),
    "done_rows3": _xa(9, 250, "rows3", n_new=3, invariant=True, done=[0, 1, 0]),
    "done_group2": _xa(4, 250, "group2", kv_group=2, invariant=True, done=[0, 1]),
    "done_var_plain": _xa(4, 250, "plain", lens=XA_LENS, done=[0, 0, 1, 0]),
})

N_CTX = 448
N_PAST = [0, 1, 62, 63, 64, 127, 128, 440]       # 1, 2 and 7 chunks of 64 keys, both sides of a chunk's end
# name -> (n_new, slots)
SELF_CASES = {f"{'slots' if sl else 'plain'}_n{n}": (n, sl) for n in (1, 2, 8) for sl in (False, True)}

_cache = {}


def _seed(family, name, pattern):
    return [ord(ch) for ch in family + name + pattern]


def xa_slices(p):
    """the key slices launch_cross_attn cuts a CROSS_CASES entry into"""
    return xattn_split(p["M"], 2, p["t_len"]) if p["variant"] in ("split", "group_split") else 1


def make(family, name, pattern):
    """(case, reference [R][d], needle weights [R][H]) of one named case, built once and shared; treat as read-only"""
    key = (family, name, pattern)
    if key not in _cache:
        seed = _seed(*key)
        if family == "encoder":
            B, T, H, lens, _ = ENCODER_CASES[name]
            c = encoder_case(seed, pattern, B, T, H, lens)
        elif family == "cross":
            p = CROSS_CASES[name]
            c = cross_case(seed, pattern, p["M"], p["n_new"], p["t_len"], p["kv_group"], p["lens"], xa_slices(p))
        else:
            n_new, slots = SELF_CASES[name]
            c = self_case(seed, pattern, N_PAST, n_new, N_CTX, slots)
        ref, w = reference(c, weights=True)
        for a in (c.q, c.K, c.V, ref, w):
            a.setflags(write=False)
        _cache[key] = (c, ref, w)
    return _cache[key]
