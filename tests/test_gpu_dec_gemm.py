"""The decoder GEMM family (launch_dec_gemm: five epilogues, the plain / ln / pn / split-K operand forms, the statistics producer,
six work shapes) and the kernels in front of it (fold_ln, repack_tiled, tiled_rowsum, embed, the tiled LayerNorm) against the
float64 reference of tests/dec_gemm_ref.py, through ohw_dbg_dec_gemm / ohw_dbg_embed / ohw_dbg_layernorm on caller data.

Every table line runs on the exact inputs (raw words must equal the reference's) and on the real ones (every element within its
derived bound; the worst error / bound per form is printed).  Output buffers are pre-filled with a sentinel and carry guard
space: every element the contract does not name must still hold the sentinel afterwards, and pad rows of tiled inputs hold NaN.
The work shape is steered with M, N, K and cu_budget alone and asserted from shape_out.

GELU lines on the exact inputs: the pre-activation is exact but the GELU is not, so they are held to the GELU term of the bound
alone (2e-6 max(1, |v|), one ulp of the output) instead of word equality.
"""
import ctypes as C

import numpy as np
import pytest

import dec_gemm_ref as R
from dec_gemm_ref import BIAS_T, GELU_T, LN, LOGITS, PLAIN, PN, QKV, RESID, S1x1, S1x2, S1x6, S2x1, S2x2, S4x2, case

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NCTX = 12
_P5 = [0, 11, 4, 12, 7]                                   # n_new = 1: position 12 == n_ctx is not stored
_P2 = [4, 9]                                              # n_new = 3: 9 + 3 == n_ctx, the last position of the cache
_P14 = [0, 9, 10, 3, 5, 1, 8, 2, 9, 6, 10, 0, 7, 4]       # 10 + 2 == n_ctx: the window's last token is not stored
_P40 = [(7 * i) % 13 for i in range(40)]                  # 0 .. 12


def _qkv(form, M, cu, shape, n_new=1, K=128):
    past = {(5, 1): _P5, (6, 3): _P2, (42, 3): _P14, (40, 1): _P40}[(M, n_new)]
    return case(QKV, form, M, 384, K, cu=cu, shape=shape, n_new=n_new, n_past=past, n_ctx=NCTX)


# Every line is derived from dec_gemm_pick (decode.hip), with mt = ceil(M / 16) m-tiles, nt = ceil(N / 16) n-tiles and
# cus = cu_budget or 256:
#   RESID plain  1x1 when mt == 1 or nt * mt <= 2 cus;  else with mt > 2 and nt * ceil(mt / 2) > 2 cus: 4x2 (K <= 1280) or
#                1x6 (K > 1280), neither with stat_out;  else 1x2.  Split-K always takes 1x2.
#   ln, pn       mt <= 2: 1x1 when nt * mt <= cus, else 2x1 when ceil(nt / 2) * mt <= cus or mt == 1
#   ln           then 4x2 when mt > 2 and ceil(nt / 2) * ceil(mt / 2) > 2 cus;  then 2x2 when nt > cus;  else 1x2
#   pn           then 2x2 when nt > cus;  else 1x2
#   plain QKV / BIAS_T / GELU_T   1x2
#   LOGITS       2x1 when mt == 1;  4x2 when mt > 2, K <= 1280 and nt * ceil(mt / 2) > 2 cus;  else 2x2
# K walks the unroll tiers of the K loop: dec_gemm_kernel with one n-tile 20 / 10 / 5 / 1 k-blocks per wave and pass
# (K = 5152: 161 blocks, 2656: 83, 1312: 41, 96: 3), with more n-tiles 5 / 1 (2048, 1312; 544, 96), the rows kernel 20 / 4 / 1
# (5152; 1312); the ln forms hold at most five blocks per wave (K = 192: two waves have none; 320; 1280: all five).
TABLE = [
    # ---- RESID, plain tiles
    case(RESID, PLAIN, 5, 48, 96, shape=S1x1, ld=56),
    case(RESID, PLAIN, 20, 48, 96, shape=S1x1),
    case(RESID, PLAIN, 5, 48, 1312, shape=S1x1),
    case(RESID, PLAIN, 5, 48, 2656, shape=S1x1),
    case(RESID, PLAIN, 20, 48, 5152, shape=S1x1),
    case(RESID, PLAIN, 19, 80, 96, cu=2, shape=S1x2, ld=88),             # nt * mt = 10 > 4
    case(RESID, PLAIN, 19, 80, 5152, cu=2, shape=S1x2),
    case(RESID, PLAIN, 40, 80, 96, cu=2, shape=S4x2, ld=88),             # 5 n-tiles: the second workgroup holds one real tile
    case(RESID, PLAIN, 40, 80, 96, cu=6, shape=S1x2),                    # 15 > 12, 10 <= 12
    case(RESID, PLAIN, 40, 80, 96, shape=S1x1),
    case(RESID, PLAIN, 40, 48, 1312, cu=2, shape=S1x6),                  # 3 m-tiles in a workgroup of six
    case(RESID, PLAIN, 100, 48, 1312, cu=2, shape=S1x6),                 # 7 m-tiles: a second workgroup with one
    case(RESID, PLAIN, 40, 48, 5152, cu=2, shape=S1x6),
    case(RESID, PLAIN, 40, 48, 1312, cu=3, shape=S1x2),                  # 9 > 6, 6 <= 6
    case(RESID, PLAIN, 40, 48, 1312, shape=S1x1),
    # ---- RESID producers of the post-norm path (x16_out, stat_out)
    case(RESID, PLAIN, 5, 64, 96, stat=True, shape=S1x1),
    case(RESID, PLAIN, 19, 64, 1312, cu=2, stat=True, shape=S1x2),
    case(RESID, PLAIN, 40, 64, 96, cu=2, stat=True, shape=S1x2),         # mt > 2: the producer keeps 1x2
    # ---- split-K (12 k-blocks: 5 does not divide them)
    case(RESID, PLAIN, 19, 80, 384, ksplit=2, shape=S1x2, ld=88),
    case(RESID, PLAIN, 19, 80, 384, ksplit=3, shape=S1x2),
    case(RESID, PLAIN, 40, 80, 384, ksplit=5, shape=S1x2),               # two row blocks
    # ---- ln forms
    case(BIAS_T, LN, 5, 192, 192, shape=S1x1, ld=200),
    case(BIAS_T, LN, 20, 192, 320, shape=S1x1),
    case(BIAS_T, LN, 5, 192, 320, cu=8, shape=S2x1),                     # 12 > 8, 6 <= 8
    case(BIAS_T, LN, 5, 80, 192, cu=4, shape=S2x1, ld=88),               # 5 n-tiles: the last workgroup holds one
    case(BIAS_T, LN, 20, 192, 320, cu=16, shape=S2x1),                   # 24 > 16, 12 <= 16
    case(BIAS_T, LN, 20, 192, 320, cu=4, shape=S2x2),                    # 12 > 4 twice, nt > cus
    case(BIAS_T, LN, 40, 192, 1280, cu=2, shape=S4x2),                   # 6 * 2 > 4
    case(BIAS_T, LN, 40, 192, 320, cu=8, shape=S2x2),                    # 12 <= 16, 12 > 8
    case(BIAS_T, LN, 40, 192, 192, shape=S1x2),
    case(GELU_T, LN, 5, 192, 1280, shape=S1x1),
    case(GELU_T, LN, 5, 192, 192, cu=8, shape=S2x1),
    case(GELU_T, LN, 40, 192, 320, cu=2, shape=S4x2),
    case(GELU_T, LN, 40, 192, 192, cu=8, shape=S2x2),
    case(GELU_T, LN, 40, 192, 1280, shape=S1x2),
    _qkv(LN, 5, 0, S1x1),
    _qkv(LN, 6, 8, S2x1, n_new=3),                                       # 24 > 8, 12 > 8, mt == 1
    _qkv(LN, 42, 2, S4x2, n_new=3),
    _qkv(LN, 40, 16, S2x2),                                              # 12 * 2 <= 32, 24 > 16
    _qkv(LN, 42, 0, S1x2, n_new=3),
    # ---- pn forms (K = 64: most lanes merge no statistics tile; 544: 34 tiles, two lanes merge two; 2048: all 128)
    case(BIAS_T, PN, 5, 192, 64, shape=S1x1, ld=200),
    case(BIAS_T, PN, 20, 192, 2048, shape=S1x1),
    case(BIAS_T, PN, 5, 192, 544, cu=8, shape=S2x1),
    case(BIAS_T, PN, 5, 80, 544, cu=4, shape=S2x1, ld=88),
    case(BIAS_T, PN, 20, 192, 544, cu=16, shape=S2x1),
    case(BIAS_T, PN, 20, 192, 544, cu=4, shape=S2x2),
    case(BIAS_T, PN, 20, 192, 544, shape=S1x1),
    case(BIAS_T, PN, 40, 192, 2048, cu=8, shape=S2x2),
    case(BIAS_T, PN, 40, 192, 544, shape=S1x2),
    case(GELU_T, PN, 5, 192, 544, shape=S1x1),
    case(GELU_T, PN, 5, 192, 64, cu=8, shape=S2x1),
    case(GELU_T, PN, 40, 192, 544, cu=8, shape=S2x2),
    case(GELU_T, PN, 40, 192, 2048, shape=S1x2),
    _qkv(PN, 5, 0, S1x1),
    _qkv(PN, 6, 8, S2x1, n_new=3),
    _qkv(PN, 42, 16, S2x2, n_new=3, K=544),
    _qkv(PN, 40, 0, S1x2),
    # ---- the 16-bit epilogues on plain tiles
    case(BIAS_T, PLAIN, 19, 80, 96, shape=S1x2, ld=88),
    case(GELU_T, PLAIN, 19, 192, 96, shape=S1x2),
    _qkv(PLAIN, 6, 0, S1x2, n_new=3),
    # ---- LOGITS: 13 n-tiles, the last with 8 real columns
    case(LOGITS, PLAIN, 5, 200, 96, shape=S2x1, ld=216),
    case(LOGITS, PLAIN, 6, 200, 96, n_new=3, shape=S2x1, ld=216),
    case(LOGITS, PLAIN, 20, 200, 1312, shape=S2x2, ld=216),
    case(LOGITS, PLAIN, 42, 200, 96, n_new=3, shape=S2x2, ld=216),
    case(LOGITS, PLAIN, 42, 200, 96, n_new=3, cu=2, shape=S4x2, ld=216),  # 13 * 2 > 4
    case(LOGITS, PLAIN, 40, 200, 544, cu=2, shape=S4x2, ld=216),
]
IDS = [R.case_name(c) for c in TABLE]
WORST = {}       # (form, dtype) -> worst error / bound on the real inputs


def _form_of(c):
    return "split-K" if c["ksplit"] > 1 else "stat-producer" if c["stat"] else R.FORM_NAMES[c["form"]]


def test_table_covers_every_shape_and_form():
    """a later change of dec_gemm_pick that re-routes a line fails that line's shape assertion; this keeps the table itself whole"""
    assert len(set(IDS)) == len(IDS)
    assert {c["shape"] for c in TABLE} == {S1x1, S2x1, S1x2, S2x2, S4x2, S1x6}
    assert {_form_of(c) for c in TABLE} == {"plain", "ln", "pn", "split-K", "stat-producer"}
    assert {c["epi"] for c in TABLE} == {QKV, BIAS_T, GELU_T, RESID, LOGITS}
    reach = {(c["epi"], c["form"], c["shape"]) for c in TABLE}
    for epi in (QKV, BIAS_T, GELU_T):
        assert {s for e, f, s in reach if (e, f) == (epi, LN)} == {S1x1, S2x1, S1x2, S2x2, S4x2}
        assert {s for e, f, s in reach if (e, f) == (epi, PN)} == {S1x1, S2x1, S1x2, S2x2}
        assert {s for e, f, s in reach if (e, f) == (epi, PLAIN)} == {S1x2}
    assert {s for e, f, s in reach if e == RESID} == {S1x1, S1x2, S4x2, S1x6}
    assert {s for e, f, s in reach if e == LOGITS} == {S2x1, S2x2, S4x2}
    for K, line in ((5152, S1x1), (2656, S1x1), (1312, S1x1), (5152, S1x6), (1312, S1x6)):
        assert any(c["K"] == K and c["shape"] == line for c in TABLE)


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from openhush_amd import engine
    engine.lib()
    return engine


def _td(dt):
    return torch.bfloat16 if dt == 0 else torch.float16


def _dev(a, td=torch.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device="cuda", dtype=td)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _tiles(x, td):
    """activation tiles of x [M][K]; the pad rows of the last tile hold NaN"""
    M, K = x.shape
    buf = torch.full((R.tiled_elems(M, K),), float("nan"), device="cuda", dtype=td)
    buf[torch.from_numpy(R.act_tiled_index(M, K)).cuda()] = _dev(x, td)
    return buf


def _guarded(a):
    """f32 rows with three NaN rows behind them"""
    return _dev(np.concatenate([a, np.full((R.GUARD_ROWS,) + a.shape[1:], np.nan)]))


def _words(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu().numpy().view(np.uint16 if t.element_size() == 2 else np.uint32)


def _want_words(a, dt, f32):
    return np.asarray(a, dtype=np.float32).view(np.uint32) if f32 else R.bits_T(R.round_T(a, dt), dt)


def launch(E, c, I, dt, cu=None, slab=None, ticket=None):
    """one ohw_dbg_dec_gemm on the inputs I -> (name -> output tensor, shape_out)"""
    td = _td(dt)
    M, K, form = c["M"], c["K"], c["form"]
    held = dict(w=_dev(I.w), bias=_dev(I.bias), gamma=_dev(I.gamma), beta=_dev(I.beta),
                x=_guarded(I.x) if form == LN else _tiles(I.x, td), stat_in=_guarded(I.stat) if form == PN else None)
    out = {k: _dev(a, torch.float32 if (R.out_is_f32(c) and k == "out") or k == "stat_out" else td) for k, a in R.images(c, I).items()}
    shape = C.c_int32(-1)
    io = E.DbgDecGemmIO(dtype=dt, epilogue=c["epi"], form=form, M=M, N=c["N"], K=K, n_new=c["n_new"], ld_out=c["ld"],
                        cu_budget=c["cu"] if cu is None else cu, ksplit=c["ksplit"], w=_ptr(held["w"]), bias=_ptr(held["bias"]),
                        gamma=_ptr(held["gamma"]), beta=_ptr(held["beta"]), x=_ptr(held["x"]), stat_in=_ptr(held["stat_in"]),
                        out=_ptr(out["out"]), slab=_ptr(slab), slab_bytes=0 if slab is None else slab.numel() * 4, ticket=_ptr(ticket),
                        x16_out=_ptr(out.get("x16_out")), stat_out=_ptr(out.get("stat_out")), k_cache=_ptr(out.get("k_cache")),
                        v_cache=_ptr(out.get("v_cache")), shape_out=C.pointer(shape))
    if c["epi"] == QKV:
        past = np.ascontiguousarray(c["n_past"], dtype=np.int32)
        io.n_past, io.d_model, io.n_head, io.n_ctx = E._ip(past), c["d_model"], c["n_head"], c["n_ctx"]
    rc = E.lib().ohw_dbg_dec_gemm(C.byref(io), _stream())
    if rc not in (0, E.OHW_E_INVALID_ARG):
        pytest.exit(f"{R.case_name(c)}: the device reported an error ({E.last_error()}): nothing more is launched", 3)
    assert rc == 0, (R.case_name(c), E.last_error())
    torch.cuda.synchronize()
    return out, shape.value


def check(c, I, dt, kind, out, tag):
    """the output images against the reference: words on the exact inputs, bounds on the real ones, the sentinel everywhere else"""
    exact = kind == "exact"
    v, bound = R.forward(c, I, dt, round_y=exact, exact=exact)
    if exact and c["form"] == PN and c["epi"] != GELU_T:
        assert R.pn_exact_margin(I, v, dt).all()           # a precondition of the inputs, not of the kernel
    want = R.place(c, R.images(c, I), v)
    lim = R.place(c, {k: np.zeros_like(a) for k, a in R.images(c).items()}, bound)
    worst = 0.0
    for k in ("out", "k_cache", "v_cache"):
        if k not in want:
            continue
        f32 = R.out_is_f32(c)
        if exact and c["epi"] != GELU_T:
            bad = np.argwhere(_words(out[k]) != _want_words(want[k], dt, f32))
            assert len(bad) == 0, (tag, k, len(bad), bad[:4].tolist())
        else:
            got = out[k].double().cpu().numpy()
            err = np.abs(got - want[k])
            ok = err <= lim[k]                              # a NaN fails; where the contract names nothing the bound is 0: the sentinel
            assert ok.all(), (tag, k, int((~ok).sum()), np.argwhere(~ok)[:4].tolist(), float(np.nanmax(err / np.maximum(lim[k], 1e-300))))
            named = lim[k] > 0
            worst = max(worst, float((err[named] / lim[k][named]).max()))
    if c["stat"]:
        M, N = c["M"], c["N"]
        stored = out["out"].double().cpu().numpy()[:M, :N]
        x16, st, st_lim = R.producer_expect(c, stored, dt)
        assert (_words(out["x16_out"]) == R.bits_T(x16, dt)).all(), tag       # the stored rows rounded once; pad rows untouched
        got = out["stat_out"].double().cpu().numpy()
        assert (got[M:] == R.SENTINEL).all(), tag
        ratio = np.abs(got[:M] - st) / st_lim
        assert (ratio <= 1.0).all(), (tag, float(ratio.max()))
        if exact:
            # integers: the sum and the mean (sixteenths) are exact, the deviations (sixteenths below 2^12) too; their squares
            # are multiples of 1 / 256 and stay exact, with every partial sum, while 256 m2 < 2^24
            assert (got[:M, :, 0] == st[:, :, 0]).all(), tag
            small = st[:, :, 1] * 256 < 2 ** 24
            assert (got[:M, :, 1][small] == st[:, :, 1][small]).all(), tag
        else:
            print(f"dec_gemm {tag}: statistics worst error / bound {ratio.max():.3f}")
    return worst


def _report(c, dt, worst):
    key = (_form_of(c), "bf16" if dt == 0 else "f16")
    WORST[key] = max(WORST.get(key, 0.0), worst)
    print(f"dec_gemm {R.case_name(c)} {key[1]}: worst error / bound {worst:.3f}; form {key[0]} so far {WORST[key]:.3f}")


def _ks_scratch(c, fill):
    tiles = (c["N"] + 15) // 16 * ((c["M"] + 31) // 32)
    return torch.full((tiles * c["ksplit"] * 512,), fill, device="cuda"), torch.zeros(tiles + 8, device="cuda", dtype=torch.int32)


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("c", TABLE, ids=IDS)
def test_table_line(E, c, kind, dt):
    I = R.make(c, kind, dt)
    slab, ticket = _ks_scratch(c, float("nan")) if c["ksplit"] > 1 else (None, None)
    out, shape = launch(E, c, I, dt, slab=slab, ticket=ticket)
    assert shape == c["shape"], (R.case_name(c), R.SHAPE_NAMES[shape], R.SHAPE_NAMES[c["shape"]])
    worst = check(c, I, dt, kind, out, f"{R.case_name(c)} {kind} dt {dt}")
    if ticket is not None:
        assert not ticket.any()
    if kind == "real":
        _report(c, dt, worst)


# the same data under different CU budgets: (case, [(cu, shape) ...]).  The four-tile form needs K <= 1280 and the rows kernel
# K > 1280, so RESID comes as two groups that both hold 1x1 and 1x2
INVARIANT = [
    (case(RESID, PLAIN, 40, 80, 96, ld=88), [(0, S1x1), (6, S1x2), (2, S4x2)]),
    (case(RESID, PLAIN, 40, 48, 1312), [(0, S1x1), (3, S1x2), (2, S1x6)]),
    (case(BIAS_T, LN, 20, 192, 320), [(0, S1x1), (16, S2x1), (4, S2x2)]),           # MT = 1, 1, 2
    (case(GELU_T, LN, 20, 192, 320), [(0, S1x1), (16, S2x1), (4, S2x2)]),
    (case(BIAS_T, PN, 20, 192, 544), [(0, S1x1), (16, S2x1), (4, S2x2)]),
    (_qkv(PN, 6, 0, None, n_new=3), [(0, S1x1), (8, S2x1)]),
    (_qkv(LN, 40, 0, None), [(0, S1x2), (16, S2x2), (2, S4x2)]),
]


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("c,runs", INVARIANT, ids=[R.case_name(c) for c, _ in INVARIANT])
def test_bits_do_not_depend_on_the_cu_budget(E, c, runs, dt):
    """what batch invariance and CU-masked streams rest on: only cu_budget changes between the runs, the bits do not"""
    I = R.make(c, "real", dt)
    first = None
    for cu, want_shape in runs:
        out, shape = launch(E, c, I, dt, cu=cu)
        assert shape == want_shape, (cu, R.SHAPE_NAMES[shape], R.SHAPE_NAMES[want_shape])
        words = {k: _words(t) for k, t in out.items()}
        if first is None:
            first = words
            check(c, I, dt, "real", out, f"{R.case_name(c)} cu {cu} dt {dt}")
        for k in words:
            assert (words[k] == first[k]).all(), (R.case_name(c), k, cu)


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("ks,M", [(2, 19), (3, 19), (5, 40)])
def test_split_k_repeats_its_bits_and_rearms_the_tickets(E, ks, M, dt):
    c = case(RESID, PLAIN, M, 80, 384, ksplit=ks, ld=88)
    I = R.make(c, "real", dt)
    slab, ticket = _ks_scratch(c, float("nan"))
    a, shape = launch(E, c, I, dt, slab=slab, ticket=ticket)
    assert shape == S1x2 and not ticket.any()
    _report(c, dt, check(c, I, dt, "real", a, f"split-K {ks} dt {dt}"))
    b, _ = launch(E, c, I, dt, slab=slab, ticket=ticket)          # the same slab and tickets again
    assert not ticket.any()
    assert (_words(a["out"]) == _words(b["out"])).all()


def _refused(E, rc, word):
    assert rc == E.OHW_E_INVALID_ARG, rc
    assert word in E.last_error(), E.last_error()


def test_rejections_launch_nothing(E):
    """every refusal comes before any device work: the buffer behind every pointer is far too small for the stated sizes and is
    still whole afterwards"""
    buf = torch.full((256,), R.SENTINEL, device="cuda")
    p = buf.data_ptr()
    past = np.zeros(4, dtype=np.int32)

    def call(**kw):
        a = dict(dtype=0, epilogue=RESID, form=PLAIN, M=19, N=80, K=96, n_new=1, ld_out=80, cu_budget=0, ksplit=0, w=p, bias=p, x=p, out=p)
        a.update(kw)
        return E.lib().ohw_dbg_dec_gemm(C.byref(E.DbgDecGemmIO(**a)), None)

    _refused(E, call(K=48), "multiple of 32")
    _refused(E, call(epilogue=BIAS_T, form=LN, K=1344), "exceeds the 1280")
    _refused(E, call(epilogue=BIAS_T, form=LN, K=96), "multiple of 64")
    _refused(E, call(epilogue=BIAS_T, form=PN, K=2080, stat_in=p), "n_stat")
    _refused(E, call(N=48, ld_out=48, x16_out=p, stat_out=p), "stat_out: N = 48")
    _refused(E, call(ksplit=4, slab=p, slab_bytes=1 << 20, ticket=p), "exceeds the K / 32")            # 3 k-blocks
    _refused(E, call(K=384, ksplit=2, slab=p, slab_bytes=5 * 2 * 2048 - 4, ticket=p), "slab_bytes")     # a short slab
    _refused(E, call(epilogue=BIAS_T, K=384, ksplit=2, slab=p, slab_bytes=1 << 20, ticket=p), "RESID epilogue only")
    _refused(E, call(epilogue=RESID, form=LN, K=128), "ln and pn forms")
    _refused(E, call(ld_out=79), "ld_out")
    _refused(E, call(epilogue=GELU_T, N=80), "multiple of 32")
    _refused(E, call(epilogue=LOGITS, M=5, n_new=3), "multiple of n_new")
    q = dict(epilogue=QKV, form=LN, M=4, N=384, K=128, k_cache=p, v_cache=p, n_past=E._ip(past), d_model=128, n_head=2, n_ctx=NCTX)
    past[2] = NCTX + 1
    _refused(E, call(**q), "n_past[2] = 13")
    past[2] = -1
    _refused(E, call(**q), "n_past[2] = -1")
    past[2] = 0
    _refused(E, call(**dict(q, n_head=3)), "d_model")
    _refused(E, call(gamma=p), "gamma and beta")
    torch.cuda.synchronize()
    assert (buf == R.SENTINEL).all()


@pytest.mark.parametrize("dt", [0, 1])
def test_chain_embed_producer_consumer(E, dt):
    """embedding -> RESID producer -> pn consumer on the very buffers the first two publish, as a decoder layer chains them"""
    td = _td(dt)
    rng = np.random.default_rng(5 + dt)
    M, n_new, d, V, P = 21, 3, 96, 50, 16
    tok = np.array([0, 17, 33, 49, 15, 16, 31, 32, 48, 1, 47, 2, 18, 34, 49, 0, 20, 40, 5, 25, 45], dtype=np.int32)     # all four 16-row tiles
    past = np.array([0, 13, 5, 2, 9, 13, 7], dtype=np.int32)                                                            # 13 + 3 == n_pos
    emb = R.round_T(rng.standard_normal((V, d)), dt)
    pos = rng.standard_normal((P, d)).astype(np.float32)
    x = torch.full((M + R.GUARD_ROWS, d), R.SENTINEL, device="cuda")
    x16 = torch.full((R.tiled_elems(M, d) + R.GUARD_TILE,), R.SENTINEL, device="cuda", dtype=td)
    stat = torch.full((M + R.GUARD_ROWS, d // 16, 2), R.SENTINEL, device="cuda")
    demb, dpos = _dev(emb), _dev(pos)
    rc = E.lib().ohw_dbg_embed(dt, demb.data_ptr(), V, dpos.data_ptr(), P, E._ip(tok), E._ip(past), x.data_ptr(), x16.data_ptr(), stat.data_ptr(),
                               M, n_new, d, _stream())
    assert rc == 0, E.last_error()
    torch.cuda.synchronize()
    rows = np.repeat(past, n_new) + np.tile(np.arange(n_new), M // n_new)
    want_x = emb[tok].astype(np.float32) + pos[rows]                                   # ONE fp32 addition: the definition, bit for bit
    got_x = x.cpu().numpy()
    assert (got_x[:M].view(np.uint32) == want_x.view(np.uint32)).all() and (got_x[M:] == R.SENTINEL).all()

    def published(x_rows, what):
        """x16 and stat against the fp32 rows they were made from"""
        c = case(RESID, PLAIN, M, d, d, stat=True)
        w16, st, st_lim = R.producer_expect(c, x_rows.astype(np.float64), dt)
        assert (_words(x16) == R.bits_T(w16, dt)).all(), what
        got = stat.double().cpu().numpy()
        ratio = np.abs(got[:M] - st) / st_lim
        print(f"dec_gemm chain {what} dt {dt}: statistics worst error / bound {ratio.max():.3f}")
        assert (ratio <= 1.0).all() and (got[M:] == R.SENTINEL).all(), what

    published(got_x[:M], "embed")

    # the producer adds a projection to x in place and republishes x16 and stat
    c = case(RESID, PLAIN, M, d, d, stat=True)
    I = R.make(c, "real", dt, seed=1)
    I.resid = got_x[:M].astype(np.float64)
    dw, db, da = _dev(I.w), _dev(I.bias), _tiles(I.x, td)
    shape = C.c_int32(-1)
    io = E.DbgDecGemmIO(dtype=dt, epilogue=RESID, form=PLAIN, M=M, N=d, K=d, n_new=1, ld_out=d, w=dw.data_ptr(), bias=db.data_ptr(), x=da.data_ptr(),
                        out=x.data_ptr(), x16_out=x16.data_ptr(), stat_out=stat.data_ptr(), shape_out=C.pointer(shape))
    assert E.lib().ohw_dbg_dec_gemm(C.byref(io), _stream()) == 0, E.last_error()
    torch.cuda.synchronize()
    assert shape.value == S1x1
    v, bound = R.forward(c, I, dt)
    got_o = x.cpu().numpy()
    err = np.abs(got_o[:M].astype(np.float64) - v)
    assert (err <= bound).all() and (got_o[M:] == R.SENTINEL).all()
    published(got_o[:M], "producer")

    # the consumer reads x16 and stat as they lie; reference: LN(out) of the fp32 rows, float64
    c2 = case(BIAS_T, PN, M, 80, d, ld=88)
    I2 = R.make(c2, "real", dt, seed=2)
    I2.x = got_o[:M].astype(np.float64)
    dw2, db2, dg2, dbe2 = _dev(I2.w), _dev(I2.bias), _dev(I2.gamma), _dev(I2.beta)
    out = _dev(R.images(c2)["out"], td)
    io = E.DbgDecGemmIO(dtype=dt, epilogue=BIAS_T, form=PN, M=M, N=80, K=d, n_new=1, ld_out=88, w=dw2.data_ptr(), bias=db2.data_ptr(),
                        gamma=dg2.data_ptr(), beta=dbe2.data_ptr(), x=x16.data_ptr(), stat_in=stat.data_ptr(), out=out.data_ptr(),
                        shape_out=C.pointer(shape))
    assert E.lib().ohw_dbg_dec_gemm(C.byref(io), _stream()) == 0, E.last_error()
    torch.cuda.synchronize()
    assert shape.value == S1x1
    v, bound = R.forward(c2, I2, dt)
    # the consumer multiplies the 16-bit copy: every x_k is off by 2^-9 / 2^-12 relative, rstd * sum |x_k w'_k| of it at most
    xr = I2.x
    rstd = 1.0 / np.sqrt(xr.var(axis=1) + R.EPS)
    bound = bound + R.HALF[dt] * (1 + R.ULP[dt]) * rstd[:, None] * (np.abs(xr) @ np.abs(R.folded(I2)[0]).T)
    want = R.place(c2, R.images(c2), v)
    lim = R.place(c2, {"out": np.zeros_like(want["out"])}, bound)
    err = np.abs(out.double().cpu().numpy() - want["out"])
    assert (err <= lim["out"]).all(), float((err / np.maximum(lim["out"], 1e-300)).max())
    print(f"dec_gemm chain consumer dt {dt}: worst error / bound {(err[:M, :80] / bound).max():.3f}")


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("tiled", [0, 1])
def test_layernorm_launch(E, tiled, dt):
    td = _td(dt)
    worst = 0.0
    for d in (64, 384, 1280, 2048):
        for rows in (1, 5, 18):
            rng = np.random.default_rng([d, rows, dt])
            x = (rng.uniform(0.5, 3.0, size=(rows, 1)) * (rng.standard_normal((rows, d)) + rng.standard_normal((rows, 1)))).astype(np.float32)
            gamma = rng.standard_normal(d).astype(np.float32)
            beta = rng.standard_normal(d).astype(np.float32)
            y, bound = R.layernorm_ref(x.astype(np.float64), gamma.astype(np.float64), beta.astype(np.float64), dt)
            if tiled:
                want = np.full(R.tiled_elems(rows, d) + R.GUARD_TILE, R.SENTINEL)
                lim = np.zeros_like(want)
                idx = R.act_tiled_index(rows, d)
                want[idx], lim[idx] = y, bound
            else:
                want = np.full((rows + R.GUARD_ROWS, d), R.SENTINEL)
                lim = np.zeros_like(want)
                want[:rows], lim[:rows] = y, bound
            dx, dg, db = _guarded(x), _dev(gamma), _dev(beta)
            out = _dev(np.full(want.shape, R.SENTINEL), td)
            rc = E.lib().ohw_dbg_layernorm(dt, dx.data_ptr(), dg.data_ptr(), db.data_ptr(), out.data_ptr(), rows, d, tiled, _stream())
            assert rc == 0, E.last_error()
            torch.cuda.synchronize()
            err = np.abs(out.double().cpu().numpy() - want)
            assert (err <= lim).all(), (d, rows, float((err / np.maximum(lim, 1e-300)).max()))
            worst = max(worst, float((err[lim > 0] / lim[lim > 0]).max()))
    print(f"layernorm tiled {tiled} dt {dt}: worst error / bound {worst:.3f}")
    buf = torch.zeros(64, device="cuda")
    p = buf.data_ptr()
    for d, t in ((2052, 0), (6, 0), (48, 1)):
        assert E.lib().ohw_dbg_layernorm(dt, p, p, p, p, 1, d, t, None) == E.OHW_E_INVALID_ARG


def test_embed_refuses_bad_tables(E):
    buf = torch.zeros(64, device="cuda")
    p = buf.data_ptr()
    i32 = lambda a: E._ip(np.ascontiguousarray(a, dtype=np.int32))

    def emb(tok, past, n_new=1, d=64, V=50, P=16):
        return E.lib().ohw_dbg_embed(0, p, V, p, P, i32(tok), i32(past), p, None, None, len(tok), n_new, d, None)
    _refused(E, emb([0, 50], [0, 0]), "tok[1] = 50")
    _refused(E, emb([0, -1], [0, 0]), "tok[1] = -1")
    _refused(E, emb([0, 1, 2], [14], n_new=3), "n_past[0] = 14")
    _refused(E, emb([0, 1, 2], [0, 0], n_new=2), "multiple of n_new")
    _refused(E, emb([0], [0], d=48), "multiple of 32")
