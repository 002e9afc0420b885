"""The all-rows output of the decoder GEMM's LOGITS epilogue (DecGemmParams::out_all; what ohw_state_score's replay reads),
through ohw_dbg_logits_rows, in both kernels that carry the epilogue: dec_gemm_kernel and the held-weights rows form.  On
integer inputs every fp32 result is exact whatever the summation order (tests/dec_gemm_ref.py), so every word of out_all must
equal the float64 reference; out keeps its last-row-per-window words, bit-equal to a launch without out_all; nothing is written
behind row M or column N."""
import ctypes as C

import numpy as np
import pytest

import dec_gemm_ref as R
from dec_gemm_ref import LOGITS, PLAIN, S2x1, S2x2, S4x2, case

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

S4x6 = 6            # kernels.hpp DG_SHAPE_4x6: dec_gemm_rows_kernel<LOGITS, 4 n-tiles, two passes of three m-tiles>
K = 96
# dec_gemm_pick (decode.hip), LOGITS, mt = ceil(M / 16), nt = ceil(N / 16), cus = cu_budget or 256:
#   2x1 when mt == 1;  the rows form 4x6 when cu_budget > 0, mt > 2, nt * ceil(mt / 2) > 2 cus and 32 <= ceil(nt / 4) <= 16 cus;
#   4x2 when mt > 2 and nt * ceil(mt / 2) > 2 cus;  else 2x2.
# ceil(nt / 4) >= 32 needs nt >= 125, that is N >= 1985; 16 cus >= 32 needs a budget of 2: the smallest of both
TABLE = [
    (case(LOGITS, PLAIN, 8, 1003, K, n_new=8, ld=1012), S2x1),
    (case(LOGITS, PLAIN, 8 * 13, 1003, K, n_new=8, ld=1012), S2x2),                 # 7 m-tiles, the last with 8 rows; 63 n-tiles, the last with 11 columns
    (case(LOGITS, PLAIN, 8 * 13, 1003, K, n_new=8, ld=1012, cu=2), S4x2),
    (case(LOGITS, PLAIN, 8 * 13, 1985, K, n_new=8, ld=1992, cu=2), S4x6),           # 125 n-tiles, the last with one column
    (case(LOGITS, PLAIN, 8 * 13, 1985, K, n_new=8, ld=1992, cu=1), S4x2),           # one CU fewer: 32 workgroups are more than 16 rounds
]
IDS = [R.case_name(c) for c, _ in TABLE]
GUARD_ROWS, LD_PAD = 3, 8


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from openhush_amd import engine
    assert hasattr(engine.lib(), "ohw_dbg_logits_rows")
    return engine


def _td(dt):
    return torch.bfloat16 if dt == 0 else torch.float16


def _dev(a, td=torch.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device="cuda", dtype=td)


def _tiles(x, td):
    M, Kx = x.shape
    buf = torch.full((R.tiled_elems(M, Kx),), float("nan"), device="cuda", dtype=td)
    buf[torch.from_numpy(R.act_tiled_index(M, Kx)).cuda()] = _dev(x, td)
    return buf


def _words(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _launch(E, c, I, dt, all_rows):
    """-> (out [windows + guard][ld], out_all [M + guard][ld + pad] or None, the shape that ran)"""
    td = _td(dt)
    M, N = c["M"], c["N"]
    held = dict(w=_dev(I.w), bias=_dev(I.bias), x=_tiles(I.x, td))
    out = _dev(R.images(c)["out"])
    ld_all = c["ld"] + LD_PAD
    out_all = torch.full((M + GUARD_ROWS, ld_all), R.SENTINEL, device="cuda") if all_rows else None
    shape = C.c_int32(-1)
    g = E.DbgDecGemmIO(dtype=dt, epilogue=LOGITS, form=PLAIN, M=M, N=N, K=c["K"], n_new=c["n_new"], ld_out=c["ld"], cu_budget=c["cu"],
                       w=held["w"].data_ptr(), bias=held["bias"].data_ptr(), x=held["x"].data_ptr(), out=out.data_ptr(),
                       shape_out=C.pointer(shape))
    io = E.DbgLogitsRowsIO(g=g, out_all=None if out_all is None else out_all.data_ptr(), ld_all=ld_all if all_rows else 0)
    rc = E.lib().ohw_dbg_logits_rows(C.byref(io), torch.cuda.current_stream().cuda_stream)
    if rc not in (0, E.OHW_E_INVALID_ARG):
        pytest.exit(f"{R.case_name(c)}: the device reported an error ({E.last_error()}): nothing more is launched", 3)
    assert rc == 0, (R.case_name(c), E.last_error())
    torch.cuda.synchronize()
    return out, out_all, shape.value


def test_the_table_reaches_both_kernels():
    assert {s for _, s in TABLE} == {S2x1, S2x2, S4x2, S4x6}


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("c,want_shape", TABLE, ids=IDS)
def test_all_rows_on_exact_inputs(E, c, want_shape, dt):
    I = R.make(c, "exact", dt)
    M, N, n_new = c["M"], c["N"], c["n_new"]
    v, _ = R.forward(c, I, dt, round_y=True, exact=True)              # [M][N], every value an integer below 2^24
    plain, none, shape0 = _launch(E, c, I, dt, all_rows=False)
    out, out_all, shape = _launch(E, c, I, dt, all_rows=True)
    assert none is None and shape0 == shape == want_shape, (R.case_name(c), shape0, shape, want_shape)
    # every word of out_all, and the sentinel behind row M and column N
    want_all = np.full((M + GUARD_ROWS, c["ld"] + LD_PAD), R.SENTINEL)
    want_all[:M, :N] = v
    bad = np.argwhere(_words(out_all) != want_all.astype(np.float32).view(np.uint32))
    assert len(bad) == 0, (R.case_name(c), len(bad), bad[:4].tolist())
    # out: the last row of each window, the sentinel elsewhere - and the same words with and without out_all
    want = R.place(c, R.images(c), v)["out"]
    assert (_words(out) == want.astype(np.float32).view(np.uint32)).all()
    assert (_words(out) == _words(plain)).all()
    assert (_words(out)[:M // n_new, :N] == _words(out_all)[n_new - 1:M:n_new, :N]).all()


@pytest.mark.parametrize("dt", [0, 1])
def test_out_all_holds_the_same_bits_in_both_kernels_on_real_inputs(E, dt):
    """real (Gaussian) inputs: out_all's rows are the same bits whichever kernel ran, and out is its last row per window"""
    c2, c6 = TABLE[4][0], TABLE[3][0]
    I = R.make(c2, "real", dt)
    out2, all2, s2 = _launch(E, c2, I, dt, all_rows=True)
    out6, all6, s6 = _launch(E, c6, I, dt, all_rows=True)
    assert (s2, s6) == (S4x2, S4x6)
    assert (_words(all2) == _words(all6)).all() and (_words(out2) == _words(out6)).all()
    M, N, n_new = c2["M"], c2["N"], c2["n_new"]
    assert (_words(out6)[:M // n_new, :N] == _words(all6)[n_new - 1:M:n_new, :N]).all()
    v, bound = R.forward(c2, I, dt)
    err = np.abs(all6.double().cpu().numpy()[:M, :N] - v)
    assert (err <= bound).all(), float((err / bound).max())


def test_refusals(E):
    c = TABLE[0][0]
    g = E.DbgDecGemmIO(dtype=0, epilogue=R.RESID, form=PLAIN, M=8, N=1003, K=K, n_new=8, ld_out=1012)
    assert E.lib().ohw_dbg_logits_rows(C.byref(E.DbgLogitsRowsIO(g=g, out_all=None, ld_all=0)), None) == E.OHW_E_INVALID_ARG
    assert "LOGITS" in E.last_error()
    g.epilogue = LOGITS
    assert E.lib().ohw_dbg_logits_rows(C.byref(E.DbgLogitsRowsIO(g=g, out_all=0x1000, ld_all=1000)), None) == E.OHW_E_INVALID_ARG
    assert "ld_all" in E.last_error()
    assert E.lib().ohw_dbg_logits_rows(None, None) == E.OHW_E_INVALID_ARG
    assert c["n_new"] == 8
