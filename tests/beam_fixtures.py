"""Crafted logits rows and beam states for test_gpu_beam_step.py.  test_beam_ref_cpu.py checks, on the reference alone, that
every fixture meets the gap conditions that make an exact comparison with the fp32 kernels fair.

Values: noise is N(0, 1) clipped to +-3 and rounded to multiples of 2^-10, planted values and the bias are multiples of 2^-10
too, so logits = v - bias is exact and the device's fp32 logits + bias gives v back bit for bit: the run with a bias and the
run without one see the same rows and must give the same result.

top-k geometry (beam_topk_kernel): a row is cut into 8 slices of per = ceil(V / 8) tokens; lane t of slice q holds the indices
q * per + t + 256 * u, u < 26."""
import numpy as np

import beam_ref as R

Q = 2.0 ** -10
FORBIDDEN = 30.0            # a value above every planted one, put on tokens the filter must drop


def noise(seed, V) -> np.ndarray:
    x = np.clip(np.random.default_rng(seed).standard_normal(V), -3.0, 3.0)
    return (np.round(x / Q) * Q).astype(np.float32)


def make_bias(V, seed=77) -> np.ndarray:
    return (np.random.default_rng(seed).integers(-24, 25, V) * 0.25).astype(np.float32)


def plant(v, idxs, top=None, values=None):
    """idxs in rank order: top, top - 1, ... (default: the lowest planted value is 11 = 8 above the noise), or explicit values"""
    idxs = [int(i) for i in idxs]
    assert len(set(idxs)) == len(idxs)
    if values is None:
        top = 11.0 + len(idxs) - 1 if top is None else top
        values = [top - c for c in range(len(idxs))]
    for i, x in zip(idxs, values):
        v[i] = x
    return v


def text_hist(seed, n):
    return [int(t) for t in np.random.default_rng(seed).integers(1000, 40000, n)]


# ------------------------------------------------------------------------------------------------ (a) top-k rows
def topk_rows(vo: R.Vocab, K: int):
    """-> list of dict(name, hist, v [V] f32, spaced): spaced rows hold planted values 1.0 apart, 8 above the noise"""
    V, tb, eot = vo.n_vocab, vo.ts_begin, vo.eot
    per = (V + 7) // 8
    K1 = K + 1
    idx = lambda q, t, u: q * per + t + 256 * u
    H3 = [tb, 50, 51]
    rows = []
    base = noise(1000 + V + K, V)

    def add(name, hist, idxs=None, spaced=False, values=None, top=None, forbidden=(), extra=None):
        v = base.copy()
        if idxs is not None:
            plant(v, idxs, top=top, values=values)
        for f in forbidden:
            v[f] = FORBIDDEN
        if extra:
            extra(v)
        rows.append(dict(name=name, hist=list(hist), v=v, spaced=spaced))

    fills = [idx(4, 10 + c, c) for c in range(K1)]
    add("one_lane", H3, [idx(2, 37, 3 + o) for o in (3, 0, 6, 1, 5, 2, 4)], spaced=True)      # 7 in one lane: a list 5 deep loses one
    add("one_wave", H3, [idx(3, 64 + 9 * c, (5 * c) % 25) for c in range(K1)], spaced=True)
    add("one_slice", H3, [idx(5, (c * 67 + 13) % 256, (c * 7) % 25) for c in range(K1)], spaced=True)
    add("one_per_slice", H3, [idx((3 * c + 1) % 8, 5 + c, c + 2) for c in range(K1)], spaced=True)
    add("edge_0_1", H3, [per, per - 1] + fills[:K - 1], spaced=True)
    add("edge_6_7", H3, [7 * per - 1, 7 * per] + fills[:K - 1], spaced=True)
    add("ends", H3, [eot - 1, 0, eot] + fills[:K - 2], spaced=True)          # index 0, eot - 1, and the last allowed text id
    HT = [50, 51, tb]                                                           # closing timestamp: end-of-text or timestamps only
    b63 = 7 * per + 63 + 256 * 20
    assert b63 >= tb and b63 + 1 < V
    add("ts_ends", HT, [V - 1, tb, tb + 1] + [tb + 700 + c for c in range(K - 2)], spaced=True)
    add("ts_lane_boundary", HT, [b63 + 1, b63, b63 + 256] + [tb + 700 + c for c in range(K - 2)], spaced=True)
    add("ts_forced_over_text", H3, [tb + 5 + 97 * c for c in range(K1)], spaced=True)
    T = 11.0 + K1
    add("tie2_slices", H3, [idx(6, 3, 1), idx(1, 200, 7)] + fills[:K - 1], values=[T, T] + [T - 1 - c for c in range(K - 1)])
    add("tie3_slices", H3, [idx(7, 9, 2), idx(3, 100, 4), idx(0, 77, 0)] + fills[:K - 1], values=[T] * 3 + [T - 1 - c for c in range(K - 1)])
    add("tie_one_lane", H3, [idx(4, 200, 9), idx(4, 200, 2), idx(4, 200, 20)] + fills[:K - 1], values=[T] * 3 + [T - 1 - c for c in range(K - 1)])
    # K + 2 equal values in one lane: the lowest K + 1 indices are due (an insertion that lets a later equal value pass keeps the highest)
    add("tie_one_lane_cut", H3, [idx(1, 99, 2 + 3 * c) for c in range(K + 2)], values=[T] * (K + 2))
    # a timestamp tied with a text token below the best text token (were it the best, the timestamp mass would win)
    add("tie_ts_text", H3, fills[:K - 1] + [tb + 30, 30000], values=[T - c for c in range(K - 1)] + [T - K + 1] * 2)
    for name, tok in (("sot", vo.sot), ("lang", vo.sot + 8), ("lang_last", vo.sot + vo.n_langs), ("no_ts", vo.no_ts), ("nosp", vo.nosp),
                      ("translate", vo.translate), ("transcribe", vo.transcribe), ("prev", vo.prev), ("solm", vo.solm)):
        add("forbidden_" + name, H3, fills, spaced=True, forbidden=[tok])
    add("last_seen", [tb + 700, 50, 51], [tb + 700 + 13 * c for c in range(K1)], spaced=True, forbidden=[tb + 699])
    add("few_forced", [50, 51, tb + 1499], [tb + 1499, V - 1], top=14.0, forbidden=[7000])        # 2 tokens remain
    add("few_unforced", [50, 51, tb + 1499], [eot, tb + 1499, V - 1], values=[20.0, 14.0, 13.0], forbidden=[7000])   # 3 remain

    def mass(v):
        v[tb + 100:tb + 300] = 8.0              # log(200) + 8 = 13.298; none alone beats the text token
    add("mass_forced", H3, fills, top=13.125, extra=mass)
    add("mass_unforced", H3, fills, top=13.5, extra=mass)
    # the window's first step
    add("initial_blank", [], fills, spaced=True, forbidden=[vo.blank] if vo.blank >= 0 else [])
    add("initial_eot", [], fills, spaced=True, forbidden=[eot])
    add("initial_ts_late", [], fills[:K] + [tb + 50], spaced=True, forbidden=[tb + 51, tb + 200])
    # histories
    add("last_ts_penult_text", [50, tb + 5], [tb + 5 + 4 * c for c in range(K1)], spaced=True, forbidden=[7000, tb + 3])
    add("last_ts_penult_ts", [tb + 2, tb + 5], fills, spaced=True, forbidden=[tb + 100])
    add("hist60_ts_at_0", [tb + 900] + text_hist(5, 59), [tb + 900 + c for c in range(K1)], spaced=True, forbidden=[tb + 899])
    h300 = text_hist(6, 300)
    h300[5], h300[290] = tb + 800, tb + 400        # the LAST timestamp counts (position 290), not the largest
    add("hist300_last_ts", h300, [tb + 400 + 50 * c for c in range(K1)], spaced=True, forbidden=[tb + 399])
    return rows


def pack_topk(vo: R.Vocab, prm: R.Params, K: int, rows):
    """rows grouped by history length into windows of K rows (padded with noise rows) -> (state, v [R][V], names [R])"""
    groups = {}
    for r in rows:
        groups.setdefault(len(r["hist"]), []).append(r)
    packed = []
    for n, g in sorted(groups.items()):
        while len(g) % K:
            g.append(dict(name="pad", hist=text_hist(len(g), n), v=noise(len(g) + n, vo.n_vocab), spaced=False))
        packed += g
    W = len(packed) // K
    st = R.new_state(W, K, prm)
    for r, row in enumerate(packed):
        n = len(row["hist"])
        st["tokens"][r, :n] = row["hist"]
        st["n_cur"][r // K] = n
        st["n_past_w"][r // K] = min(n + 2, prm.n_text_ctx - 2)
    return st, np.stack([r["v"] for r in packed]), [r["name"] for r in packed]


# ------------------------------------------------------------------------------------------------ (b) update windows
TOP = 20.0          # planted top value of the update fixtures: the noise holds 2e-4 of the mass


def _std_row(base, toks):
    return plant(base.copy(), toks, top=TOP)


def _steep_row(base, toks):
    return plant(base.copy(), toks, values=[TOP] + [TOP - 8.0 - c for c in range(len(toks) - 1)])


def _window(vo, K, seed, n_cur=3, P=None, bs=None, rows=None, fin_cnt=0, done=0, hists=None):
    """one window: dict(n_cur, P, hists [K], v [K][V], bs [K], fin_cnt, fin_tok, fin_len, fin_sum, done, kv_seed)"""
    rng = np.random.default_rng(seed)
    base = noise(seed, vo.n_vocab)
    if hists is None:
        hists = [[vo.ts_begin] + text_hist(seed * 10 + j, n_cur - 1) if n_cur else [] for j in range(K)]
    if rows is None:
        rows = [_std_row(base, text_hist(seed * 10 + 5 + j, K + 1)) for j in range(K)]
    if bs is None:
        bs = [-0.3 * j for j in range(K)]
    fin_len = [int(x) for x in rng.integers(1, 9, K)]
    return dict(n_cur=n_cur, P=n_cur + 2 if P is None else P, hists=hists, v=np.stack(rows), bs=list(bs), fin_cnt=fin_cnt,
                fin_tok=[text_hist(seed + 50 + f, fin_len[f]) for f in range(K)], fin_len=fin_len,
                fin_sum=[-1.25 * (f + 1) for f in range(K)], done=done, kv_seed=seed, base=base)


def far(K, lead):
    """beam sums: `lead` for the first beams, the others far below, all on a 0.3 lattice so that no two scores come close"""
    return list(lead) + [-10.0 - 0.3 * j for j in range(len(lead), K)]


def update_launches(vo: R.Vocab, K: int):
    """-> list of dict(name, first, n_max, windows [2], expect): every launch holds two windows with different states"""
    tb, eot, V = vo.ts_begin, vo.eot, vo.n_vocab
    toks = lambda s, n=K + 1: text_hist(s, n)
    wins = []

    def case(name, **kw):
        w = _window(vo, K, 100 + len(wins), **kw)
        w["name"] = name
        wins.append(w)
        return w

    # all K new beams from beam 0
    case("one_source", bs=far(K, [0.0]))
    # a full permutation of the sources: new beam i continues beam perm[i]
    perm = {2: [1, 0], 3: [2, 0, 1], 5: [3, 0, 4, 1, 2]}[K]
    bs = [0.0] * K
    for i, j in enumerate(perm):
        bs[j] = -0.3 * i
    w = case("permutation", bs=bs)
    w["v"] = np.stack([_steep_row(w["base"], toks(900 + j)) for j in range(K)])
    w["perm"] = perm
    # end-of-text among the best: the best candidate of beam 0 (and of beam 1), with the pool at 0, K - 1 and K entries
    for n_eot in (1, 2):
        for fin in (0, K - 1, K):
            w = case(f"eot{n_eot}_pool{fin}", bs=far(K, [0.0, -0.3]), fin_cnt=fin)
            for j in range(n_eot):
                t = toks(910 + j)
                w["v"][j] = _std_row(w["base"], [eot] + t[:K])
    # end-of-text ranked below the K-th live candidate: it must not enter the pool
    w = case("eot_below_cut", bs=far(K, [0.0]))
    w["v"][0] = _std_row(w["base"], toks(920)[:K] + [eot])
    # exact ties: bit-identical rows with equal sums in two beams (their histories and kv_slot rows differ: the source shows)
    a, b = (0, 1) if K == 2 else (1, 2)
    lead = [-0.5, -0.5] if K == 2 else [0.0, -0.5, -0.5]
    w = case("tie_inside", bs=far(K, lead))
    w["v"][b] = w["v"][a]
    if K > 2:
        lead = [0.0, -(K - 2) - 0.5, -(K - 2) - 0.5]        # beam 0 gives K - 1 beams, the tied pair competes for the last one
        w = case("tie_at_cut", bs=far(K, lead))
        w["v"][b] = w["v"][a]
    # the dead-beam state: one live beam, K - 1 at -inf (duplicates of it), a filter that leaves end-of-text and one timestamp
    hd = [50, 51, tb + 1500]
    w = case("dead_beams", bs=[-1.0] + [-np.inf] * (K - 1), hists=[hd] * K)
    row = w["base"].copy()
    row[eot], row[V - 1], row[7000] = 10.0, 8.0, FORBIDDEN
    w["v"] = np.stack([row] * K)
    # a finished window beside a live one (both orders), and the three length limits
    plain = lambda: case("plain")
    launches = []
    pairs = [(wins[i], wins[i + 1]) for i in range(0, len(wins) - 1, 2)]
    if len(wins) % 2:
        pairs.append((wins[-1], plain()))
    for x, y in pairs:
        launches.append(dict(name=x["name"] + "+" + y["name"], first=False, n_max=220, windows=[x, y]))
    d1, d2 = case("done", done=1, fin_cnt=1, bs=far(K, [-2.0])), case("done", done=1, fin_cnt=1, bs=far(K, [-2.0]))
    launches.append(dict(name="done+live", first=False, n_max=220, windows=[d1, plain()], n_done=0, done_after=[1, 0]))
    launches.append(dict(name="live+done", first=False, n_max=220, windows=[plain(), d2], n_done=0, done_after=[0, 1]))
    launches.append(dict(name="end_n_max", first=False, n_max=8, windows=[case("n_max", n_cur=7), plain()], n_done=1, done_after=[1, 0]))
    launches.append(dict(name="end_max_tokens", first=False, n_max=1000, windows=[plain(), case("max_tokens", n_cur=447, P=120)], n_done=1,
                         done_after=[0, 1]))
    launches.append(dict(name="end_text_ctx", first=False, n_max=220, windows=[case("text_ctx", n_cur=20, P=446), plain()], n_done=1,
                         done_after=[1, 0]))
    # the first step: one logits row per window, only beam 0 proposes; different prompt lengths
    f1, f2 = case("first_a", n_cur=0, P=2), case("first_b", n_cur=0, P=3)
    f1["v"] = np.stack([plant(f1["base"].copy(), toks(930)[:K - 1] + [tb + 20, toks(931)[0]], top=TOP)])
    f1["v"][0][eot] = FORBIDDEN
    f2["v"] = np.stack([plant(f2["base"].copy(), toks(932), top=TOP)])
    f2["v"][0][tb + 51] = FORBIDDEN
    launches.append(dict(name="first_step", first=True, n_max=220, windows=[f1, f2], n_done=0, done_after=[0, 0]))
    return launches


def pack_update(vo: R.Vocab, prm: R.Params, K: int, windows, first):
    """-> (state, v [W or R][V]) of a launch"""
    W = len(windows)
    st = R.new_state(W, K, prm)
    vs = []
    for w, x in enumerate(windows):
        rng = np.random.default_rng(x["kv_seed"])
        st["n_cur"][w], st["n_past_w"][w], st["win_done"][w], st["fin_cnt"][w] = x["n_cur"], x["P"], x["done"], x["fin_cnt"]
        for j in range(K):
            r = w * K + j
            st["tokens"][r, :x["n_cur"]] = x["hists"][j]
            st["beam_sum"][r] = x["bs"][j]
            st["kv_slot"][r] = rng.integers(0, W * K, prm.n_text_ctx)
            st["fin_tok"][r, :x["fin_len"][j]] = x["fin_tok"][j]
            st["fin_len"][r] = x["fin_len"][j]
            st["fin_sum"][r] = x["fin_sum"][j]
        vs.append(x["v"][:1] if first else x["v"])
    return st, np.concatenate(vs)


# ------------------------------------------------------------------------------------------------ (c) a chained run
CHAIN_W, CHAIN_K, CHAIN_STEPS = 3, 5, 14
CHAIN_RULER = (1, 2, 4, 8, 13, 21, 31, 45, 66, 81, 97, 123, 148, 182)       # Mian-Chowla
CHAIN_UNIT = 0.003
CHAIN_TOP = 30.0                # the noise holds 1e-8 of the mass: rows with different allowed sets share their log-sum-exp
CHAIN_P0 = (2, 2, 436)          # window 2 reaches the end of the text context at its 11th step


def chain_params(vo):
    return R.default_params(n_max=CHAIN_STEPS)


def chain_row(vo: R.Vocab, noise_w, w: int, hist):
    """the logits row of a beam: a fixed function of (window, token history).  Planted peaks, 1 + CHAIN_UNIT * CHAIN_RULER[s]
    apart at step s.  With one spacing for all steps, two paths that took their second-best tokens at different steps would tie
    in exact arithmetic and differ by rounding alone; the ruler (a Sidon sequence: all pairwise sums differ) keeps the
    cumulative scores of such paths whole units apart.
      window 0: end-of-text joins the peaks from step 4 on: its pool fills
      window 1: a timestamp joins the peaks at steps 3 and 8 (timestamp pairs follow); nothing ends it but n_max
      window 2: at step 3 the timestamp 30.00 s outweighs everything; at step 4 the beams whose last text token is odd get -inf
                on it: end-of-text is all they can propose, so fewer than K continuations survive; it runs into the text context"""
    tb, eot, V = vo.ts_begin, vo.eot, vo.n_vocab
    s = len(hist)
    v = noise_w.copy()
    sp = 1.0 + CHAIN_UNIT * CHAIN_RULER[s]
    rng = np.random.default_rng([w] + [int(t) for t in hist])
    n = CHAIN_K + 2
    heights = [CHAIN_TOP - c * sp for c in range(n)]
    closing = s >= 2 and hist[-1] >= tb and hist[-2] < tb
    if closing:
        last = hist[-1]
        ts = [min(last + o, V - 1) for o in (0, 3, 7, 12, 18, 25, 33)]
        ts = sorted(set(ts))
        if w == 2 and last == V - 1 and hist[-2] % 2 == 1:
            v[V - 1] = -np.inf
        else:
            plant(v, ts, values=heights[:len(ts)])
        return v
    toks = [int(t) for t in rng.choice(np.arange(1000, 45000), n, replace=False)]
    plant(v, toks, values=heights)
    half = CHAIN_TOP - 0.5 * sp         # half a slot: the scores stay on the half-unit lattice
    if w == 0 and s >= 4:
        v[eot] = half
    if w == 1 and s in (3, 8):
        v[tb + 100 + 40 * s] = half
    if w == 2 and s == 3:
        plant(v, [V - 1] + [tb + 1400 + c for c in range(n - 1)], values=[CHAIN_TOP + 8.0] + heights[1:])
    return v


def chain_start(vo, prm):
    st = R.new_state(CHAIN_W, CHAIN_K, prm)
    st["n_past_w"][:] = CHAIN_P0
    return st


def chain_logits(vo, noises, st, first):
    K = CHAIN_K
    rows = []
    for w in range(CHAIN_W):
        for j in range(1 if first else K):
            r = w * K + j
            if st["win_done"][w]:               # never read
                rows.append(noises[w])
                continue
            rows.append(chain_row(vo, noises[w], w, [int(t) for t in st["tokens"][r, :st["n_cur"][w]]]))
    return np.stack(rows)


def chain_noises(vo):
    return [noise(4000 + w, vo.n_vocab) for w in range(CHAIN_W)]


def run_chain(vo, stepper):
    """the chained run: stepper(first, state, logits, side) -> the next state, fed back; the double buffers alternate as in
    ohw_beam_search (the first step reads side 0).  Yields (step, state)"""
    prm = chain_params(vo)
    noises = chain_noises(vo)
    st = chain_start(vo, prm)
    for s in range(CHAIN_STEPS):
        logits = chain_logits(vo, noises, st, s == 0)
        st = stepper(s == 0, st, logits, s & 1)
        yield s, st
