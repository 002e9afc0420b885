"""Crafted logits rows and sampler states for test_gpu_sampler_rows.py.  test_sampler_ref_cpu.py checks, on the reference
alone, that every fixture meets the distance conditions that make an exact comparison with the fp32 kernels fair.

Values as in beam_fixtures: noise is N(0, 1) clipped to +-3 on multiples of 2^-10, planted values and the bias lie on the same
grid, so logits = v - bias is exact and the device's fp32 logits + bias gives v back bit for bit.

Geometry (sampler_kernel and both phases of sampler_t_row, openhush_amd/csrc/decode.hip), the same for V = 51865 and 51866:
  phase 1: 8 slices of PER = ceil(V / 8) = 6484 tokens; thread t of slice q loads q * PER + t + 512 * u, u < 13; threads
           t >= 340 are masked at u = 12 (6144 + 340 = PER)
  phase 2: 8 wave ranges of WPER = 6528 = 102 tiles of 64, walked in batches of 16 tiles: a full wave's 7th batch holds 6 tiles
           (from WPER-relative 6144 on); the last wave has 6144 + V % 64 tokens, its last tile 25 or 26 live lanes
  every timestamp lies in the last slice and in the last wave's range (ts_begin >= 7 * WPER)."""
import numpy as np

import beam_fixtures as F
import sampler_ref as S

PER, WPER = 6484, 6528
WIN, RUN = 11.0, 10.0           # a greedy row's winner (8 above the noise) and its runner-up
TOP = 20.0                      # a ladder's planted value: at T <= 1 the noise holds about 1e-5 of the mass
TEMPS = (0.2, 0.6, 1.0)


def idx(q, t, u):
    return q * PER + t + 512 * u


def H3(vo):
    """text and timestamps both allowed"""
    return [vo.ts_begin, 50, 51]


def HT(vo, k=0):
    """a closing timestamp: only end-of-text and the timestamps from ts_begin + k on remain"""
    return [50, 51, vo.ts_begin + k]


def base_noise(vo):
    return F.noise(7000 + vo.n_vocab, vo.n_vocab)


# ------------------------------------------------------------------------------------------------ (h) the -inf masks
def inf_masks(vo):
    """name -> indices that hold -inf: index 0 (thread 0's first load), one thread's whole column of slice 2 (t = 17, all 13
    loads), the row's noise maximum, two of the ladder's positions, about 20 more; "hist" adds nosp (rows with a history)"""
    base = base_noise(vo)
    rng = np.random.default_rng(99)
    m = {0, 64, WPER, int(np.argmax(base))} | {idx(2, 17, u) for u in range(13)}
    m |= {int(i) for i in rng.integers(100, vo.eot - 1, 16)} | {int(i) for i in rng.integers(vo.ts_begin + 60, vo.n_vocab - 1, 6)}
    return {"first": sorted(m), "hist": sorted(m | {vo.nosp})}


def effective(row, vo):
    """the row the sampler sees: v with -inf where the row's mask has it"""
    v = row["v"].copy()
    if row.get("mask"):
        v[inf_masks(vo)[row["mask"]]] = -np.inf
    return v


# ------------------------------------------------------------------------------------------------ greedy rows
def greedy_rows(vo: S.Vocab):
    """-> list of dict(name, hist, v [V] f32, tie: the decision is an exact tie by construction, mask: None / "hist" / "first")"""
    V, tb, eot = vo.n_vocab, vo.ts_begin, vo.eot
    base = base_noise(vo)
    rows = []

    def add(name, hist, win=(), values=None, forbidden=(), tie=False, mask=None, extra=None):
        v = base.copy()
        F.plant(v, win, values=values if values is not None else [WIN, RUN][:len(win)])
        for f in forbidden:
            v[f] = F.FORBIDDEN
        if extra:
            extra(v)
        rows.append(dict(name=name, hist=list(hist), v=v, tie=tie, mask=mask))

    h3, ht = H3(vo), HT(vo)
    other = idx(3, 100, 5)
    # (a) geometry: [winner, runner-up]
    add("win_0", h3, [0, other])
    add("win_per_m1", h3, [PER - 1, PER])
    add("win_per", h3, [PER, PER - 1])
    add("win_7per_m1", h3, [7 * PER - 1, 7 * PER])
    add("win_7per", h3, [7 * PER, 7 * PER - 1])
    add("win_last_live", h3, [idx(2, 339, 12), idx(3, 0, 0)])               # the last live load of slice 2, the first of slice 3
    add("win_masked_neighbour", h3, [idx(5, 339, 12), idx(5, 338, 12)])     # both in the masked 13th load
    add("win_last_wave_first", h3, [idx(4, 448, 0), idx(1, 448, 0)])
    add("one_thread_hi", h3, [idx(5, 77, 9), idx(5, 77, 2)])
    add("one_thread_lo", h3, [idx(5, 77, 2), idx(5, 77, 9)])
    add("one_wave", h3, [idx(6, 130, 4), idx(6, 150, 4)])
    add("win_eot_m1", h3, [eot - 1, other])
    add("win_eot", h3, [eot, other])
    # under a closing timestamp everything allowed lies in the last slice: the runner-up cannot be elsewhere
    add("win_ts_begin", ht, [tb, tb + 700], forbidden=[7000, eot - 1])
    add("win_last", ht, [V - 1, tb], forbidden=[7000])
    add("win_eot_closing", ht, [eot, V - 1], values=[WIN + 2.0, RUN], forbidden=[7000])        # end-of-text outweighs the timestamps
    for name, tok in (("sot", vo.sot), ("lang_first", vo.sot + 1), ("lang_last", vo.sot + vo.n_langs), ("translate", vo.translate),
                      ("transcribe", vo.transcribe), ("solm", vo.solm), ("prev", vo.prev), ("nosp", vo.nosp), ("no_ts", vo.no_ts)):
        add("forbidden_" + name, h3, [idx(4, 10, 0), idx(1, 11, 1)], forbidden=[tok])
    # (b) ties: the lowest index is owed
    add("tie2_slices", h3, [idx(6, 3, 1), idx(1, 200, 7)], values=[WIN, WIN], tie=True)
    add("tie3_slices", h3, [idx(7, 9, 2), idx(3, 100, 4), idx(0, 500, 3)], values=[WIN] * 3, tie=True)     # the lowest: wave 7 of slice 0
    add("tie_one_thread", h3, [idx(4, 200, 9), idx(4, 200, 2)], values=[WIN, WIN], tie=True)
    add("tie_ts", h3, [tb + 78, tb + 77], values=[WIN, WIN], tie=True)
    # a timestamp equal to the best text token.  The mass of all timestamps is at least that one's, so the rule stays unforced
    # only where it is the one timestamp allowed (the history's last is V - 1): log mass == best text exactly, in fp32
    # (expf(0) = 1, logf(1) = 0) as in float64, `>` is false, and text wins the tie
    add("tie_ts_text", [V - 1, 50, 51], [V - 1, 30000], values=[WIN, WIN], tie=True, forbidden=[V - 2])
    # (f) histories
    blank = [vo.blank] if vo.blank >= 0 else []
    add("hist0", [], [idx(4, 10, 0), tb + 50], forbidden=blank + [eot, tb + 51, V - 1],
        extra=lambda v: v.__setitem__(vo.nosp, F.FORBIDDEN - 1.0))                           # a no-speech probability near 0.1
    add("hist0_ts", [], [tb + 50, tb], values=[WIN + 2.0, WIN], forbidden=[tb + 51])          # forced: the last initial timestamp
    add("hist1_text", [50], [idx(4, 10, 0), other])
    add("hist1_ts", [tb + 7], [idx(4, 10, 0), other], forbidden=[tb + 5, tb + 7, tb + 100])       # a lone timestamp: text only
    add("hist2_closing", [50, tb + 5], [tb + 5, tb + 9], forbidden=[7000, tb + 3])
    add("hist2_pair", [tb + 2, tb + 5], [idx(4, 10, 0), other], forbidden=[tb + 100])
    add("hist60_ts_at_0", [tb + 900] + F.text_hist(5, 59), [tb + 900, tb + 901], forbidden=[tb + 899])
    h300 = F.text_hist(6, 300)
    h300[5], h300[290] = tb + 800, tb + 400                    # the LAST timestamp counts (position 290), not the largest
    add("hist300_last_ts", h300, [tb + 400, tb + 450], forbidden=[tb + 399])
    hmax = F.text_hist(8, 447)                                  # max_tokens - 1: the longest history the entries accept
    hmax[3], hmax[440] = tb + 900, tb + 100
    add("hist_longest", hmax, [tb + 100, tb + 101], forbidden=[tb + 99])
    # (h) -inf: values of 30.0 under the mask must neither win nor count
    under = [0, idx(2, 17, 0), idx(2, 17, 12), int(np.argmax(base))]
    add("inf_hidden_winners", h3, [idx(2, 18, 3), other], forbidden=under, mask="hist")
    add("inf_then_winner", h3, [idx(0, 0, 3), other], mask="hist")                 # thread 0 of slice 0: -inf first, the winner later
    add("inf_closing", ht, [tb, tb + 700], forbidden=[7000], mask="hist")          # slices 0..6 hold nothing allowed
    add("inf_first_step", [], [idx(4, 10, 0), tb + 50], forbidden=blank + [eot, tb + 51] + under[:2], mask="first",
        extra=lambda v: v.__setitem__(vo.nosp, F.FORBIDDEN - 1.0))
    return rows


# ------------------------------------------------------------------------------------------------ (c) the timestamp-mass rule
def mass_rows(vo: S.Vocab):
    """-> list of dict(name, hist, v, forced): beam_fixtures' pair (200 timestamps at 8.0: log mass 13.298) and a pair whose 1500
    timestamps from ts_begin + 1 on share the mass evenly (log 1500 + 6 = 13.313), against a best text token at 13.125 / 13.5"""
    tb = vo.ts_begin
    rows = []
    for r in F.topk_rows(vo, 2):
        if r["name"] in ("mass_forced", "mass_unforced"):
            rows.append(dict(name=r["name"], hist=r["hist"], v=r["v"], forced=r["name"] == "mass_forced", tie=False, mask=None))
    assert len(rows) == 2 and vo.n_vocab - (tb + 1) == 1500
    for name, top in (("even_forced", 13.125), ("even_unforced", 13.5)):
        v = base_noise(vo)
        v[tb + 1:] = 6.0
        F.plant(v, [idx(4, 10, 0), idx(1, 11, 1)], values=[top, top - 1.0])
        rows.append(dict(name=name, hist=H3(vo), v=v, forced=name == "even_forced", tie=False, mask=None))
    return rows


def mass_targets(vo, row):
    """the tokens a mass row's draws aim at (T = 1): timestamps at the ends and in the middle of the mass, and, unforced, the
    planted text tokens"""
    tb = vo.ts_begin
    ts = [tb + 100, tb + 199, tb + 299] if row["name"].startswith("mass_") else [tb + 1, tb + 750, vo.n_vocab - 1]
    text = sorted(int(i) for i in np.flatnonzero(row["v"][:vo.eot] > 10.0))
    return ts if row["forced"] else text + ts


# ------------------------------------------------------------------------------------------------ (d), (e), (h) draws
def ladder_positions(vo: S.Vocab):
    V = vo.n_vocab
    pos = [0, 63, 64, 1023, 1024, WPER - 1, WPER, 3 * WPER - 1, 3 * WPER, 7 * WPER - 1, 7 * WPER, WPER + 6143, WPER + 6144, PER - 1, PER,
           vo.eot - 1, vo.ts_begin, 7 * WPER + 6144, V - 1]
    assert len(set(pos)) == len(pos)
    return sorted(pos)


RULER = (0, 409, 1229, 205, 1843, 819, 1434, 102, 1638, 614, 1024, 307, 2048, 1331, 512, 1741, 922, 1536, 717)      # x 2^-10: 0 .. 2.0


def draw_batches(vo: S.Vocab):
    """-> list of dict(name, hist, v, T, want [n] tokens, us [n] or None, mask).  Row c of a batch draws with us[c] and must return
    want[c].  us None: the reference's own interval midpoints (sampler_ref.midpoint), filled in by with_uniforms.

    The timestamp-mass rule compares ALL timestamps with the best single text token, so three planted timestamps as heavy as
    the planted text tokens would force the rule and drop the text.  The ladders therefore hold their timestamps 1.25 T below
    their text tokens (e^-1.25 each: 0.86 of the best text token together, the rule 0.15 nat from forcing at every T), and the
    ladder of exactly equal values with u = (c + 0.5) / S is the one of the 16 text positions."""
    V, tb, eot = vo.n_vocab, vo.ts_begin, vo.eot
    base = base_noise(vo)
    pos = ladder_positions(vo)
    text = [i for i in pos if i < eot]
    ts = [i for i in pos if i >= tb]
    assert len(text) == 16 and len(ts) == 3
    out = []
    for T in TEMPS:
        drop = 1.25 * T
        # equal values, text positions: u = (c + 0.5) / S
        v = F.plant(base.copy(), text, values=[TOP] * 16)
        out.append(dict(name=f"equal_text_T{T}", hist=H3(vo), v=v, T=T, want=text, us=[(c + 0.5) / 16 for c in range(16)], mask=None))
        # every position
        v = F.plant(base.copy(), text + ts, values=[TOP] * 16 + [TOP - drop] * 3)
        out.append(dict(name=f"ladder_T{T}", hist=H3(vo), v=v, T=T, want=pos, us=None, mask=None))
        # (h) the same row under the -inf mask: three of its positions are gone
        gone = set(inf_masks(vo)["hist"])
        out.append(dict(name=f"ladder_inf_T{T}", hist=H3(vo), v=v, T=T, want=[i for i in pos if i not in gone], us=None, mask="hist"))
        # (e) a closing timestamp: end-of-text and timestamps from ts_begin + 10 on; everything the filter removes holds 30.0.
        # All that is left lies in the last wave's range, nothing below the first planted token has any probability and nothing
        # above the last: u = 2^-20 and 1 - 2^-20 owe the first and the last
        keep = [tb + 10, tb + 11, 7 * WPER + 6143, 7 * WPER + 6144, V - 2, V - 1]
        v = F.plant(base.copy(), keep, values=[TOP] * len(keep))
        v[text + [tb, tb + 9]] = F.FORBIDDEN
        out.append(dict(name=f"closing_T{T}", hist=HT(vo, 10), v=v, T=T, want=keep, us=None, mask=None))
        out.append(dict(name=f"closing_ends_T{T}", hist=HT(vo, 10), v=v, T=T, want=[keep[0], keep[-1]], us=[2.0 ** -20, 1.0 - 2.0 ** -20], mask=None))
        # (e) the first step: blank, end-of-text and timestamps past max_initial_ts go, the no-speech probability is defined
        blank = [vo.blank] if vo.blank >= 0 else []
        first_text = [i for i in text if i not in blank]
        v = F.plant(base.copy(), first_text + [tb, tb + 50], values=[TOP] * len(first_text) + [TOP - drop] * 2)
        v[blank + [eot, tb + 51, 7 * WPER + 6144, V - 1]] = F.FORBIDDEN
        v[vo.nosp] = F.FORBIDDEN - 1.0
        out.append(dict(name=f"first_step_T{T}", hist=[], v=v, T=T, want=sorted(first_text + [tb, tb + 50]), us=None, mask=None))
    # unequal planted values on a fixed ruler spanning 2.0 (T = 1: at lower T the lightest token's interval gets too narrow)
    vals = [TOP - r * F.Q for r in RULER]
    order = text + ts
    for i in range(16, 19):
        vals[i] -= 1.5                  # the timestamps: at most 3 e^-1.5 = 0.67 of the best text token
    assert RULER[0] == 0
    v = F.plant(base.copy(), order, values=vals)
    out.append(dict(name="ruler_T1.0", hist=H3(vo), v=v, T=1.0, want=pos, us=None, mask=None))
    return out


def with_uniforms(vo, prm, b):
    """the batch's uniforms: its own, or the midpoints of its wanted tokens' intervals under the reference"""
    if b["us"] is not None:
        return list(b["us"])
    _, cp, _, _, _ = S.distribution(vo, prm, effective(b, vo), None, b["hist"], b["T"])
    return [S.midpoint(cp, i) for i in b["want"]]


# ------------------------------------------------------------------------------------------------ (g) update cases
def update_launches(vo: S.Vocab):
    """-> list of dict(name, n_max, force_len, advance, rows).  rows: dict(name, hist, v, n_past, done, sum_lp); one token holds
    nearly all the mass of a row (20.0), so the arg-max and a draw with u = 0.5 pick it"""
    V, tb, eot = vo.n_vocab, vo.ts_begin, vo.eot
    base = base_noise(vo)
    k = [0]

    def row(name, hist, tok=None, n_past=5, done=0, forbidden=()):
        k[0] += 1
        v = base.copy()
        v[7000 + 13 * k[0] if tok is None else tok] = TOP
        for f in forbidden:
            v[f] = F.FORBIDDEN
        return dict(name=name, hist=list(hist), v=v, n_past=n_past, done=done, sum_lp=-0.25 * k[0])

    h3 = H3(vo)
    text = lambda n, s=0: h3 + F.text_hist(40 + s, n - 3)
    L = []
    L.append(dict(name="eot", n_max=220, force_len=0, advance=1, rows=[row("plain", h3), row("eot", h3, eot), row("eot_long", text(60), eot)]))
    L.append(dict(name="n_max", n_max=8, force_len=0, advance=1, rows=[row("at_n_max", text(7)), row("short_of_n_max", text(6, 1)), row("eot", h3, eot)]))
    L.append(dict(name="force_len", n_max=220, force_len=5, advance=1,
                  rows=[row("reaches_force_len", text(4), forbidden=[eot]), row("below_force_len", h3, forbidden=[eot]),
                        row("past_force_len", text(5), eot)]))
    L.append(dict(name="max_tokens", n_max=1000, force_len=0, advance=1, rows=[row("at_max_tokens", text(447)), row("short_of_max_tokens", text(446, 1))]))
    L.append(dict(name="text_ctx_advance0", n_max=220, force_len=0, advance=0,
                  rows=[row("at_ctx", h3, n_past=447), row("short_of_ctx", h3, n_past=446), row("plain", h3, n_past=0)]))
    L.append(dict(name="text_ctx_advance1", n_max=220, force_len=0, advance=1,
                  rows=[row("at_ctx", h3, n_past=446), row("short_of_ctx", h3, n_past=445), row("plain", h3, n_past=0)]))
    L.append(dict(name="done_beside_live", n_max=220, force_len=0, advance=1,
                  rows=[row("live", h3), row("done", text(9), done=1, n_past=17), row("eot", h3, eot), row("done_at_limits", text(447), done=1, n_past=446),
                        row("live2", text(20, 2))]))
    return L
