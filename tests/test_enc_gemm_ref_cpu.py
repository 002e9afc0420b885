"""tests/enc_gemm_ref.py on its own, no GPU: the exact inputs are exact, the reference (written from the definitions) stays inside
its own bounds when the product is emulated in fp32 through the GEMM view the kernels are given, place() is injective, and every
injected fault - an edit of the reference description, never of a kernel - breaks word equality on the exact inputs and the
bound on the real ones of at least one table line."""
import numpy as np
import pytest

import enc_gemm_ref as R

DTS = [0, 1]
LINES = list(R.TABLE)


def _words(c, v, dt):
    return v.astype(np.float32).view(np.uint32) if R.out_is_f32(c) else R.bits_T(R.round_T(v, dt), dt)


def _flush(v):
    """gelu of a large negative integer is a denormal-sized negative number: round_T models the normal range only"""
    return np.where(np.abs(v) < 1e-30, 0.0, v)


def test_table_is_the_one_the_issue_lists():
    t = R.TABLE
    g = {k: R.geometry(c) for k, c in t.items()}
    assert (g["conv1"]["M"], g["conv1"]["N"], g["conv1"]["K"], g["conv1"]["lda"], g["conv1"]["rows_per_batch"]) == (300, 256, 192, 64, 100)
    assert g["conv1"]["a_batch_stride"] == 102 * 64 and g["conv1"]["c_batch_stride"] == 102 * 256 and g["conv1"]["out_offset"] == 256
    assert (g["conv1_many"]["M"], g["conv1_many"]["N"]) == (1800, 512)
    assert (g["conv2"]["M"], g["conv2"]["lda"], g["conv2"]["K"], g["conv2"]["rows_per_batch"], g["conv2"]["c_batch_stride"]) == (350, 128, 192, 50, 50 * 256)
    assert (g["conv2_longk"]["M"], g["conv2_longk"]["K"]) == (150, 768)
    assert (g["xkv"]["M"], g["xkv"]["N"], g["xkv"]["K"], g["xkv"]["batch"], g["xkv"]["batch_offset"], g["xkv"]["n_head"]) == (300, 768, 128, 5, 2, 3)
    assert g["xkv_packed"]["M"] == 201 and g["xkv_short"]["M"] == 37 and (g["xkv_short"]["batch"], g["xkv_short"]["batch_offset"]) == (2, 1)
    for k in ("remap_bias_t", "remap_resid", "remap_f32"):
        assert (g[k]["M"], g[k]["N"], g[k]["K"], g[k]["rows_per_batch"], g[k]["c_batch_stride"]) == (300, 256, 128, 100, 104 * 256)
    for k, c in t.items():
        assert c["N"] % 256 == 0 and c["K"] % 64 == 0          # every kernel is legal for every line
        assert g[k]["M"] < 1024 or (g[k]["M"] + 255) // 256 * (c["N"] // 256) < 128        # launch_gemm's own pick is the 128x128 kernel
        # the last element any row of A reads is inside the buffer (the formula ohw_dbg_enc_gemm checks)
        nb = -(-g[k]["M"] // g[k]["rows_per_batch"])
        assert (nb - 1) * g[k]["a_batch_stride"] + (min(g[k]["M"], g[k]["rows_per_batch"]) - 1) * g[k]["lda"] + g[k]["K"] <= g[k]["a_elems"]
    # the packed map from the definition: exclusive prefix sums 0, 100, 137
    m = R.row_map(t["xkv_packed"])
    assert m[0] == 0 and m[99] == 99 and m[100] == 100 and m[136] == 136 and m[137] == 200 and m[200] == 263 and len(m) == 201


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", LINES)
def test_exact_inputs_are_exact(name, dt):
    c = R.TABLE[name]
    I = R.make(c, "exact", dt)
    for a in (I.x, I.w, I.bias) + ((I.pos,) if I.pos is not None else ()) + ((I.resid,) if I.resid is not None else ()):
        assert (a.astype(np.float32).astype(np.float64) == a).all() and (a == np.rint(a)).all()
    assert (R.round_T(I.x, dt) == I.x).all() and (R.weights(I, dt) == I.w).all()      # the 16-bit type holds the operands as they are
    assert (R.round_T(np.array([R.PAD_FILL, R.SENTINEL]), dt) == [R.PAD_FILL, R.SENTINEL]).all()
    # sum |a w| + |b| (+ |resid|) bounds every partial sum, whatever the order: integers below 2^22 are exact in fp32
    plain = dict(c, epi=R.EPI_BIAS_RESID_F32 if I.resid is not None else R.EPI_F32)       # the line before GELU, pos and the conversion
    v, bound = R.forward(plain, I, dt)
    mags = bound / ((c["K"] + 16) * R.F32)
    assert mags.max() < 2 ** 22
    assert (v == np.rint(v)).all() and (np.abs(v) <= mags).all()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", LINES)
def test_emulation_stays_inside_the_bounds(name, dt):
    """the definition (forward) against an fp32 product through the GEMM view (a_image + geometry + repack): pad channels filled
    with PAD_FILL, zero rows, overlapping rows, strides and all"""
    c = R.TABLE[name]
    for seed in range(2):
        rng = np.random.default_rng(seed)
        I = R.make(c, "exact", dt)
        v, bound = R.forward(c, I, dt, exact=True)
        got = R.emulate(c, I, dt, rng)
        if R.is_gelu(c):
            assert (np.abs(got - v) <= bound).all(), name
        else:
            assert (_words(c, got, dt) == _words(c, v, dt)).all(), name
        I = R.make(c, "real", dt)
        v, bound = R.forward(c, I, dt)
        got = R.emulate(c, I, dt, rng)
        ratio = float((np.abs(got - v) / bound).max())
        print(f"emulation {name} dt {dt} shuffle {seed}: worst error / bound {ratio:.3f}")
        assert ratio <= 1.0


@pytest.mark.parametrize("name", LINES)
def test_place_is_injective_and_inside_the_image(name):
    c = R.TABLE[name]
    idx = R.place_index(c).reshape(-1)
    assert len(np.unique(idx)) == idx.size == c["M"] * c["N"]
    assert idx.min() >= 0 and idx.max() < R.image_elems(c)
    img = R.place(c, R.images(c), np.zeros((c["M"], c["N"])))
    assert (img == R.SENTINEL).sum() == img.size - idx.size and (img[R.image_elems(c):] == R.SENTINEL).all()
    named = np.zeros(img.size, dtype=bool)
    named[idx] = True
    if name == "conv1":                      # rows 0 and 101 of every window keep the sentinel
        rows = named[:R.image_elems(c)].reshape(3, 102, 256).all(axis=2)
        assert not rows[:, 0].any() and not rows[:, 101].any() and rows[:, 1:101].all()
    if name == "xkv":                        # the slots of windows 0 and 1 keep the sentinel
        w = named[:R.image_elems(c)].reshape(4, 5, 3, 100, 64)
        assert not w[:, :2].any() and w[:, 2:].all()
    if name == "xkv_packed":                 # positions past a window's length keep the sentinel
        w = named[:R.image_elems(c)].reshape(4, 5, 3, 100, 64)
        assert w[:, 2].all() and w[:, 3, :, :37].all() and not w[:, 3, :, 37:].any() and w[:, 4, :, :64].all() and not w[:, 4, :, 64:].any()
    if name == "remap_resid":                # the 4 gap rows per window are not named
        rows = named[:R.image_elems(c)].reshape(3, 104, 256).all(axis=2)
        assert rows[:, :100].all() and not named[:R.image_elems(c)].reshape(3, 104, 256)[:, 100:].any()


# (line, forward fault, place fault, tile): tiles of 64, 128 and 256 rows are the three kernels' m-tiles
FAULTS = [
    ("conv1", "a_stride_ignored", None, 128),
    ("conv2", "a_stride_ignored", None, 128),
    ("conv1", "tile_first_window", None, 64),
    ("conv1", "tile_first_window", None, 128),
    ("conv1_many", "tile_first_window", None, 256),
    ("conv2", "tile_first_window", None, 256),
    ("conv1", None, "tile_first_window_out", 256),
    ("remap_bias_t", None, "tile_first_window_out", 256),
    ("remap_resid", None, "tile_first_window_out", 256),
    ("remap_f32", None, "tile_first_window_out", 128),
    ("conv1", None, "out_row_t", 128),
    ("conv2", "stride1", None, 128),
    ("conv2_longk", "stride1", None, 128),
    ("conv1", "taps_swapped", None, 128),
    ("conv2", "taps_swapped", None, 128),
    ("conv1", "pad_not_zeroed", None, 128),
    ("conv2", "pos_clamped", None, 128),
    ("xkv", None, "batch_offset_dropped", 128),
    ("xkv_short", None, "batch_offset_dropped", 128),
    ("xkv", None, "head_pos_swapped", 128),
    ("xkv", None, "slab_wrong_d", 128),
    ("xkv_packed", None, "slab_wrong_d", 128),
    ("xkv_packed", None, "map_ignored", 128),
    ("remap_resid", "resid_twice", None, 128),
]
LISTED = {"a_stride_ignored", "tile_first_window", "out_row_t", "stride1", "taps_swapped", "pad_not_zeroed", "pos_clamped",
          "batch_offset_dropped", "head_pos_swapped", "slab_wrong_d", "map_ignored", "resid_twice", "gelu_tanh"}


def test_every_listed_fault_is_injected():
    assert {f or p for _, f, p, _ in FAULTS} | {"gelu_tanh"} == LISTED | {"tile_first_window_out"}


def _run(c, I, dt, exact, ffault=None, pfault=None, tile=128):
    v, bound = R.forward(c, I, dt, exact=exact, fault=ffault, tile=tile)
    img = R.place(c, R.images(c, I), v, fault=pfault, tile=tile)
    lim = R.place(c, np.zeros(img.size), bound)           # the bound lies where the CONTRACT stores: zero wherever the sentinel must stay
    return img, lim


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name,ffault,pfault,tile", FAULTS, ids=[f"{n}-{f or p}-{t}" for n, f, p, t in FAULTS])
def test_each_fault_breaks_equality_and_the_bound(name, ffault, pfault, tile, dt):
    c = R.TABLE[name]
    I = R.make(c, "exact", dt)
    good, lim = _run(c, I, dt, True)
    bad, _ = _run(c, I, dt, True, ffault, pfault, tile)
    assert (_words(c, _flush(good), dt) != _words(c, _flush(bad), dt)).any(), "equality survives the fault"
    if R.is_gelu(c):                         # GELU lines are held to the exact-input bound instead of word equality
        assert float((np.abs(good - bad)[lim > 0] / lim[lim > 0]).max()) > 2.0
    I = R.make(c, "real", dt)
    good, lim = _run(c, I, dt, False)
    bad, _ = _run(c, I, dt, False, ffault, pfault, tile)
    named = lim > 0
    worst = float((np.abs(good - bad)[named] / lim[named]).max())
    spilled = int((good != bad)[~named].sum())            # elements that must keep the sentinel and do not
    print(f"fault {ffault or pfault} (tile {tile}) on {name} dt {dt}: seen, moves an element by {worst:.3g} bounds, overwrites {spilled} sentinels")
    assert worst > 2.0          # beyond the bound on both sides of the reference


@pytest.mark.parametrize("dt", DTS)
def test_gelu_by_the_tanh_formula(dt):
    """The tanh formula differs from the erf one by 1e-4 .. 4e-4 at |v| = 1 .. 3.  conv2's output is fp32 in both dtypes and sees it:
    on the exact inputs, where the bound is the GELU term alone, by a wide margin; on the real inputs it exceeds the full bound,
    whose accumulation term (208 * 2^-23 * sum |a w| = 2.5e-4) is of the size of the difference itself.  conv1's 16-bit output
    cannot resolve it (one ulp of the type is 4e-3 / 5e-4 relative) and is not asked to."""
    c = R.TABLE["conv2"]
    I = R.make(c, "exact", dt)
    good, bound = R.forward(c, I, dt, exact=True)
    bad, _ = R.forward(c, I, dt, exact=True, fault="gelu_tanh")
    exact_ratio = float((np.abs(good - bad) / bound).max())
    assert exact_ratio > 20 and (good.astype(np.float32) != bad.astype(np.float32)).any()
    I = R.make(c, "real", dt)
    good, bound = R.forward(c, I, dt)
    bad, _ = R.forward(c, I, dt, fault="gelu_tanh")
    real_ratio = float((np.abs(good - bad) / bound).max())
    print(f"fault gelu_tanh on conv2 dt {dt}: seen, moves an element by {exact_ratio:.3g} bounds (exact inputs), {real_ratio:.3g} bounds (real inputs)")
    assert real_ratio > 1.0
