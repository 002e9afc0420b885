"""tests/dec_gemm_ref.py on its own, no GPU: the claims its exact inputs rest on hold in an fp32 emulation, the reference stays
inside its own bounds, the tile maps are bijections, and every injected fault - an edit of the reference description, never of
a kernel - breaks equality on the exact inputs and, where a bound can see it, the bound on the real ones."""
import numpy as np
import pytest

import dec_gemm_ref as R

CASES = {
    "resid": R.case(R.RESID, R.PLAIN, 19, 80, 96, ld=88),
    "resid_longk": R.case(R.RESID, R.PLAIN, 5, 48, 1312),
    "bias_t_ln": R.case(R.BIAS_T, R.LN, 20, 80, 192, ld=96),
    "gelu_ln": R.case(R.GELU_T, R.LN, 5, 192, 320),
    "bias_t_pn": R.case(R.BIAS_T, R.PN, 20, 80, 544, ld=96),
    "qkv_ln": R.case(R.QKV, R.LN, 6, 384, 128, n_new=3, n_past=[4, 9], n_ctx=12),
    "qkv_pn": R.case(R.QKV, R.PN, 6, 384, 128, n_new=3, n_past=[0, 9], n_ctx=12),
    "logits": R.case(R.LOGITS, R.PLAIN, 6, 200, 96, n_new=3, ld=216),
}
DTS = [0, 1]


def _words(c, v, dt):
    return v.astype(np.float32).view(np.uint32) if R.out_is_f32(c) else R.bits_T(R.round_T(v, dt), dt)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", list(CASES))
def test_exact_inputs_are_exact_in_fp32(name, dt):
    c = CASES[name]
    I = R.make(c, "exact", dt)
    f = np.float32
    for a in (I.w, I.bias, I.x) + ((I.gamma, I.beta) if I.gamma is not None else ()) + ((I.resid,) if I.resid is not None else ()):
        assert (a.astype(f).astype(np.float64) == a).all()
    if c["form"] != R.LN:
        assert (R.round_T(I.x, dt) == I.x).all()                       # tiles of the 16-bit type hold them as they are
    W, b, _ = R.folded(I)
    assert (R.round_T(W, dt) == W).all()                                 # the folded weights survive the rounding of the repack
    assert (b.astype(f).astype(np.float64) == b).all() and np.abs(b).max() < 2 ** 24
    if c["form"] in (R.LN, R.PN):
        x = I.x.astype(f)
        s = x.sum(axis=1, dtype=f)
        assert (s.astype(np.float64) == I.x.sum(axis=1)).all()           # the fp32 sum ...
        mean = s / f(c["K"])
        assert (mean == I.mu.astype(f)).all()                            # ... the mean ...
        dev = x - mean[:, None]
        assert (np.abs(dev) == I.cdev.astype(f)[:, None]).all()          # ... and the deviations are exact
        var = (dev * dev).sum(axis=1, dtype=f) / f(c["K"])
        assert (var == (I.cdev ** 2).astype(f)).all()
        rstd = f(1) / np.sqrt(var + f(R.EPS))
        y = (dev * rstd[:, None]).astype(np.float64)
        assert (np.abs(y) < 1).all() and (np.abs(y) > 1 - 2e-5).all()
        assert (R.round_T(y, dt) == np.sign(dev)).all()                  # +-(1 - ~5e-6) rounds to exactly +-1
        st = R.tile_stats(I.x)
        assert (st[:, :, 0] == I.mu[:, None]).all() and (st[:, :, 1] == 16 * I.cdev[:, None] ** 2).all()
        for m in range(c["M"]):                                          # Chan's merge of such tiles is exact in fp32
            cnt, mu, m2 = R.merge_tiles(st[m].astype(f), dtype=f)
            assert (cnt, mu, m2) == (c["K"], I.mu[m], c["K"] * I.cdev[m] ** 2)
    v, _ = R.forward(c, I, dt, round_y=True)
    mags = np.abs(I.x if c["form"] == R.PLAIN else np.ones_like(I.x) * 16) @ np.abs(W).T + np.abs(b)
    assert mags.max() < 2 ** 22                                          # no partial sum leaves fp32's integers
    if c["form"] == R.PN:
        assert R.pn_exact_margin(I, v, dt).all()                         # rstd is inexact: the words are decided all the same
        assert (R.round_T(v, dt) == np.rint(v - 0.5) + 0.5).all()
    elif c["epi"] != R.GELU_T:
        assert (v * 2 == np.rint(v * 2)).all()                           # multiples of 1/2: gamma = 1/2 at most


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", list(CASES))
def test_emulation_stays_inside_the_bounds(name, dt):
    c = CASES[name]
    for seed in range(3):
        rng = np.random.default_rng(seed)
        I = R.make(c, "exact", dt)
        v, bound = R.forward(c, I, dt, round_y=True, exact=True)
        got = R.emulate(c, I, dt, rng)
        if c["epi"] == R.GELU_T:
            assert (np.abs(got - v) <= bound).all()
        else:
            assert (_words(c, got, dt) == _words(c, v, dt)).all(), name
        I = R.make(c, "real", dt)
        v, bound = R.forward(c, I, dt)
        got = R.emulate(c, I, dt, rng)
        ratio = float((np.abs(got - v) / bound).max())
        print(f"emulation {name} dt {dt} shuffle {seed}: worst error / bound {ratio:.3f}")
        assert ratio <= 1.0


def _run(c, I, dt, kind, **fault):
    pf = {k: v for k, v in fault.items() if k == "fault" and v in ("kv_pos_plus1", "logits_row_before")}
    ff = {} if pf else fault
    v, bound = R.forward(c, I, dt, round_y=kind == "exact", **ff)
    img = R.place(c, R.images(c, I), v, **pf)
    bimg = R.place(c, {k: np.zeros_like(a) for k, a in R.images(c).items()}, bound)
    return img, bimg


FAULTS = [
    ("resid", dict(fault="drop_kblock", kb=1)),
    ("resid_longk", dict(fault="drop_kblock", kb=40)),
    ("resid", dict(fault="twice_kblock", kb=2)),
    ("bias_t_ln", dict(fault="twice_kblock", kb=5)),
    ("bias_t_pn", dict(fault="drop_kblock", kb=16)),
    ("resid", dict(fault="swap_ntiles")),
    ("qkv_ln", dict(fault="swap_ntiles")),
    ("resid", dict(fault="skip_bias_last_tile")),
    ("logits", dict(fault="swap_ntiles")),
    ("bias_t_ln", dict(fault="skip_bias_last_tile")),
    ("bias_t_ln", dict(fault="mean_next_row")),
    ("bias_t_pn", dict(fault="mean_next_row")),
    ("bias_t_pn", dict(fault="stat_tile_twice", dup_tile=33)),
    ("qkv_pn", dict(fault="stat_tile_twice", dup_tile=0)),
    ("qkv_ln", dict(fault="kv_pos_plus1")),
    ("qkv_pn", dict(fault="kv_pos_plus1")),
    ("logits", dict(fault="logits_row_before")),
    ("resid", dict(fault="resid_twice")),
]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name,fault", FAULTS, ids=[f"{n}-{f['fault']}" for n, f in FAULTS])
def test_each_fault_breaks_equality_and_the_bound(name, fault, dt):
    c = CASES[name]
    I = R.make(c, "exact", dt)
    good, _ = _run(c, I, dt, "exact")
    bad, _ = _run(c, I, dt, "exact", **fault)
    assert any((_words(c, good[k], dt) != _words(c, bad[k], dt)).any() for k in good), "equality survives the fault"
    I = R.make(c, "real", dt)
    good, bimg = _run(c, I, dt, "real")
    bad, _ = _run(c, I, dt, "real", **fault)
    worst = max(float((np.abs(good[k] - bad[k]) / np.maximum(bimg[k], 1e-300)).max()) for k in good)
    print(f"fault {fault} on {name} dt {dt}: moves an element by {worst:.3g} bounds")
    assert worst > 2.0          # beyond the bound on both sides of the reference


@pytest.mark.parametrize("dt", DTS)
def test_gelu_by_the_tanh_formula(dt):
    """At the precision of a 16-bit output the tanh formula (at most 4.8e-4 from the erf one) hides under one ulp of the output
    (2^-8 / 2^-11 relative): no output-level bound can see it.  It breaks the GELU term itself, which is what the bound allows the
    kernel's own erf approximation: before the conversion the two differ by hundreds of GELU_TERM."""
    c = CASES["gelu_ln"]
    I = R.make(c, "real", dt)
    good, bound = R.forward(c, I, dt)
    bad, _ = R.forward(c, I, dt, fault="gelu_tanh")
    pre, _ = R.forward(dict(c, epi=R.BIAS_T), I, dt)
    term = R.GELU_TERM * np.maximum(1.0, np.abs(pre))
    assert (np.abs(good - bad) / term).max() > 50
    I = R.make(c, "exact", dt)
    good, _ = R.forward(c, I, dt, round_y=True)
    bad, _ = R.forward(c, I, dt, round_y=True, fault="gelu_tanh")
    assert (good != bad).any()


def test_tile_maps_are_bijections():
    for rows, cols in ((16, 32), (48, 96), (208, 544), (32, 2048)):
        for idx in (R.act_tiled_index(rows, cols), R.weight_tiled_index(rows, cols)):
            assert sorted(idx.reshape(-1).tolist()) == list(range(rows * cols))
    for M, d in ((5, 64), (19, 96), (40, 192)):                          # ragged M: into the buffer, no element twice
        idx = R.act_tiled_index(M, d).reshape(-1)
        assert len(set(idx.tolist())) == M * d and idx.min() >= 0 and idx.max() < R.tiled_elems(M, d)
    # the weight map read the other way round is repack_tiled's own decomposition of a destination index
    N, K = 48, 96
    idx = R.weight_tiled_index(N, K)
    for n, k in ((0, 0), (17, 33), (47, 95), (31, 64)):
        i = int(idx[n, k])
        j, lane, blk = i & 7, (i >> 3) & 63, i >> 9
        kb, nt = blk % (K // 32), blk // (K // 32)
        assert (nt * 16 + (lane & 15), kb * 32 + (lane >> 4) * 8 + j) == (n, k)


def test_rounding_helpers():
    assert R.round_T(np.array([257.0, 259.0, 1.0 + 2.0 ** -8, -3.0]), 0).tolist() == [256.0, 260.0, 1.0, -3.0]      # ties to even
    assert R.round_T(np.array([2049.0, 2051.0]), 1).tolist() == [2048.0, 2052.0]
    assert R.bits_T(np.array([1.0, -2.0, 77.0]), 0).tolist() == [0x3f80, 0xc000, 0x429a]
    assert R.bits_T(np.array([1.0, -2.0]), 1).tolist() == [0x3c00, 0xc000]
