"""Inputs, float64 reference, error bounds and output placement for the forms in which run_encode (engine.hip) launches the
encoder GEMM kernels (gemm.hip 128x128, gemm256.hip 256x256, gemm_small.hip 64x64): conv1 and conv2 as GEMMs over overlapping
rows of a padded time-major image, the head-major cross-K/V store with batch / batch_offset and the packed-row map, and the
row-major epilogues under a per-window row remap.  Plain numpy, no GPU.  The number formats, the GELU and its bound terms come
from dec_gemm_ref.py.

A table line is a dict (TABLE).  make() builds its inputs:

  exact  integers in -4 .. 4: every product and partial sum is an integer far below 2^24, so an fp32 output is THE value
         whatever the summation order and a 16-bit output is that value rounded once
  real   Gaussians; activations rounded to the 16-bit type (they are given to the kernel in it), weights left as fp32 values:
         the entry rounds them with the loader's kernels, the reference with round_T

forward() is the reference, written from the definition and not from the GEMM view:

  conv   y[b][t][n] = bias[n] + sum_{c < c_in, j < 3} w[n][c][j] * x[b][stride * t + j - 1][c],  x = 0 outside 0 .. rows - 1,
         then GELU, then + pos[t][n] for conv2
  xkv    out[slab][first + b][h][t][dh] = enc[b][t] . W[slab * d_model + 64 h + dh] + bias; packed rows carry the same values,
         window b's rows behind the exclusive prefix sum of the lengths
  remap  y[b][r] = x[b][r] W^T + bias (+ the residual)

and returns every output element before its final conversion, [M][N] in the kernel's row order m, with the bound on
|kernel - reference| next to it.  place() puts values where the contract stores them; every other element of an output image
keeps SENTINEL.  geometry() is the GEMM view of the same line - what ohw_dbg_enc_gemm is told - and a_image() the A buffer the
test uploads; emulate() multiplies through THAT view in fp32, so the CPU tests tie the two descriptions together.  The
fault-injection tests (test_enc_gemm_ref_cpu.py) edit this description through the `fault` arguments, never a kernel.
"""
import zlib

import numpy as np

from dec_gemm_ref import F32, GELU_SLOPE, GELU_TERM, HALF, SENTINEL, ULP, bits_T, gelu, gelu_tanh, round_T  # noqa: F401

EPI_BIAS_T, EPI_BIAS_GELU_T, EPI_BIAS_RESID_F32, EPI_GELU_POS_F32, EPI_F32, EPI_CROSSKV_T = range(6)     # gemm.hpp GemmEpilogue
AUTO, K128, SMALL, K256 = range(4)                                                                      # ohw.h OHW_EG_KERNEL_*
KERNEL_NAMES = ("auto", "k128", "small", "k256")
KERNEL_N = {AUTO: 128, K128: 128, SMALL: 64, K256: 256}        # N must be a multiple of
GUARD_ROWS = 3
PAD_FILL = 3.0           # channels c_in .. c_pad - 1 of the interior rows of a conv input image: the result must not see them


def _conv(epi, B, rows, T, stride, c_in, c_pad, N):
    return dict(form="conv", epi=epi, B=B, rows=rows, T=T, stride=stride, c_in=c_in, c_pad=c_pad, N=N, M=B * T, K=3 * c_pad)


def _xkv(lengths, batch, first, t_len=100, K=128, L=2, d_model=192, packed=True):
    return dict(form="xkv", epi=EPI_CROSSKV_T, lengths=list(lengths), B=len(lengths), batch=batch, first=first, t_len=t_len, K=K,
                d_model=d_model, H=d_model // 64, N=2 * L * d_model, M=sum(lengths), packed=packed)


def _remap(epi, B=3, rows=100, pitch=104, N=256, K=128):
    return dict(form="remap", epi=epi, B=B, rows=rows, T=rows, pitch=pitch, N=N, K=K, M=B * rows)


# conv1: 2 Tn = 100 (200) rows per window, none a multiple of a tile height: the window boundaries at rows 100, 200 (200 .. 1600)
# lie inside 64-, 128- and 256-row tiles and the last tile is ragged; the output goes one row down into a padded image.
# conv1_many: 1800 rows = 8 m-tiles of gemm256 = a group of 6 and a group of 2, x 2 n-tiles.  conv2: stride 2, pos[m % Tn].
# conv2_longk: 12 K-tiles.  xkv: N = 768 = 4 slabs of d_model = 192: 128- and 256-column tiles straddle slab and head boundaries.
TABLE = {
    "conv1": _conv(EPI_BIAS_GELU_T, B=3, rows=100, T=100, stride=1, c_in=40, c_pad=64, N=256),
    "conv1_many": _conv(EPI_BIAS_GELU_T, B=9, rows=200, T=200, stride=1, c_in=40, c_pad=64, N=512),
    "conv2": _conv(EPI_GELU_POS_F32, B=7, rows=100, T=50, stride=2, c_in=64, c_pad=64, N=256),
    "conv2_longk": _conv(EPI_GELU_POS_F32, B=3, rows=100, T=50, stride=2, c_in=256, c_pad=256, N=256),
    "xkv": _xkv([100, 100, 100], batch=5, first=2, packed=False),
    "xkv_packed": _xkv([100, 37, 64], batch=5, first=2),
    "xkv_short": _xkv([37], batch=2, first=1),
    "remap_bias_t": _remap(EPI_BIAS_T),
    "remap_resid": _remap(EPI_BIAS_RESID_F32),
    "remap_f32": _remap(EPI_F32),
}
for _name, _c in TABLE.items():
    _c["name"] = _name


def out_is_f32(c):
    return c["epi"] in (EPI_BIAS_RESID_F32, EPI_GELU_POS_F32, EPI_F32)


def is_gelu(c):
    return c["epi"] in (EPI_BIAS_GELU_T, EPI_GELU_POS_F32)


def row_shift(c):
    """conv1 stores output row t as image row 1 + t"""
    return 1 if c["form"] == "conv" and c["epi"] == EPI_BIAS_GELU_T else 0


def out_pitch(c):
    """rows of one window in the output image: conv1's padded image, conv2's dense rows, the remap lines' gap rows"""
    return c["pitch"] if c["form"] == "remap" else c["T"] + 2 * row_shift(c)


def window_rows(c):
    """(b [M], t [M]): the window and the row inside it of the kernel's row m.  Packed rows: window b's rows start at the
    exclusive prefix sum of the lengths"""
    if c["form"] == "xkv":
        return (np.concatenate([np.full(n, b) for b, n in enumerate(c["lengths"])]), np.concatenate([np.arange(n) for n in c["lengths"]]))
    m = np.arange(c["M"])
    return m // c["T"], m % c["T"]


def row_map(c):
    """c_row_map of a packed cross-K/V line: row m is row b * t_len + t of the unpacked windows"""
    b, t = window_rows(c)
    return (b * c["t_len"] + t).astype(np.int32)


def geometry(c):
    """the GEMM view, as run_encode sets GemmParams: the fields of ohw_dbg_enc_gemm_io, the A buffer's elements, and where in
    the output image (elements from its start) the out pointer stands"""
    N, K, M = c["N"], c["K"], c["M"]
    g = dict(M=M, N=N, K=K, conv_cin=0, ldc=N, c_batch_stride=0, d_model=0, n_head=0, t_len=0, batch=0, batch_offset=0, out_offset=0)
    if c["form"] == "conv":
        cp = c["c_pad"]
        g.update(lda=c["stride"] * cp, a_batch_stride=(c["rows"] + 2) * cp, rows_per_batch=c["T"], conv_cin=c["c_in"],
                 c_batch_stride=out_pitch(c) * N, out_offset=row_shift(c) * N, a_elems=c["B"] * (c["rows"] + 2) * cp)
    elif c["form"] == "remap":
        g.update(lda=K, a_batch_stride=c["rows"] * K, rows_per_batch=c["rows"], c_batch_stride=c["pitch"] * N, a_elems=M * K)
    else:
        g.update(lda=K, a_elems=M * K, ldc=0, d_model=c["d_model"], n_head=c["H"], t_len=c["t_len"], batch=c["batch"], batch_offset=c["first"])
        if c["packed"]:
            g.update(a_batch_stride=0, rows_per_batch=M)
        else:
            g.update(a_batch_stride=c["t_len"] * K, rows_per_batch=c["t_len"])
    return g


# ---- inputs -------------------------------------------------------------------------------------------------------------------

class Inputs:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def make(c, kind, dt, seed=0):
    """-> Inputs, float64 arrays.  conv: x [B][rows][c_in], w [N][c_in][3], pos [T][N] (conv2).  xkv: x [M][K] (the windows' rows
    end to end), w [N][K].  remap: x [M][K], w [N][K], resid [M][N] (RESID).  bias [N] everywhere.  x holds values of the 16-bit
    type; w, bias, pos and resid are fp32 values (real: w is NOT yet rounded to the type - weights() does that)"""
    rng = np.random.default_rng([zlib.crc32(c["name"].encode()), int(kind == "real"), dt, seed])
    N, M = c["N"], c["M"]
    conv = c["form"] == "conv"
    x_shape = (c["B"], c["rows"], c["c_in"]) if conv else (M, c["K"])
    w_shape = (N, c["c_in"], 3) if conv else (N, c["K"])
    fan_in = 3 * c["c_in"] if conv else c["K"]
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    I = Inputs(pos=None, resid=None)
    if kind == "exact":
        draw = lambda shape: rng.integers(-4, 5, size=shape).astype(np.float64)
        I.x, I.w, I.bias = draw(x_shape), draw(w_shape), draw(N)
    else:
        draw = lambda shape: f32(rng.standard_normal(shape))
        I.x, I.w, I.bias = round_T(rng.standard_normal(x_shape), dt), f32(rng.standard_normal(w_shape) / np.sqrt(fan_in)), draw(N)
    if c["epi"] == EPI_GELU_POS_F32:
        I.pos = draw((c["T"], N))
    if c["epi"] == EPI_BIAS_RESID_F32:
        I.resid = draw((M, N))
    return I


def weights(I, dt):
    """the weights the product sees: rounded once to the 16-bit type (convert_rows / repack_conv)"""
    return round_T(I.w, dt)


def a_image(c, I):
    """the A buffer.  conv: the time-major image [B][rows + 2][c_pad], rows 0 and rows + 1 of every window zero, the pad channels
    of the interior rows PAD_FILL.  Otherwise the rows as they are"""
    if c["form"] != "conv":
        return I.x.copy()
    img = np.zeros((c["B"], c["rows"] + 2, c["c_pad"]))
    img[:, 1:-1, :] = PAD_FILL
    img[:, 1:-1, :c["c_in"]] = I.x
    return img


def repacked(c, w16, swap=False, pad=0.0):
    """repack_conv (weights.hip): [N][c_in][3] -> [N][3][c_pad], pad channels zero.  swap: the source read as [N][3][c_in]"""
    N, c_in, cp = c["N"], c["c_in"], c["c_pad"]
    out = np.full((N, 3, cp), pad)
    out[:, :, :c_in] = w16.reshape(N, 3, c_in) if swap else w16.transpose(0, 2, 1)
    return out


# ---- the reference --------------------------------------------------------------------------------------------------------------

def _conv_sources(c, fault, tile):
    """(window [B][T][3], padded row [B][T][3]): the input row that tap j of output (b, t) reads, as a row of the zero-padded
    window (row r of x is padded row r + 1).  The definition: (b, stride * t + j).  Faults re-address the padded image as the
    flat array of rows it is in memory"""
    B, T, stride, pr = c["B"], c["T"], c["stride"], c["rows"] + 2
    b, t, j = np.meshgrid(np.arange(B), np.arange(T), np.arange(3), indexing="ij")
    if fault == "stride1":
        stride = 1
    if fault == "a_stride_ignored":           # row m = b T + t at m * lda: the windows taken as contiguous
        return np.divmod(stride * (b * T + t) + j, pr)
    if fault == "tile_first_window":          # every row of an m-tile addressed from the window of the tile's first row
        m = b * T + t
        b0 = (m // tile * tile) // T
        return np.divmod(b0 * pr + stride * (m - b0 * T) + j, pr)
    return b, stride * t + j


def forward(c, I, dt, exact=False, fault=None, tile=128):
    """-> (v [M][N], bound [M][N]): every output element before its final conversion, and the bound on |kernel - v| after it.

    Bound, per element, every term from the number formats:
      fp32 accumulation  (K + 16) * 2^-23 * (sum |a w| + |b| (+ |resid|)): at most K + 16 additions (K products into the
                         accumulator, the bias, the residual), each faithfully rounded on a partial sum no larger than the sum
                         of the magnitudes; K is the GEMM's (3 c_pad for a conv: the zero taps and pad channels count)
      GELU               GELU_SLOPE * (the above) + GELU_TERM * max(1, |v|)
      conv2's pos        + 2^-23 * (|gelu(v)| + |pos|): one more fp32 addition, after the GELU
      16-bit output      + one ulp of the type at |v| (f16: at least its subnormal step 2^-24)
    exact (the exact inputs, where only GELU lines need a bound): no accumulation term - the sums are exact.
    fault: a_stride_ignored, tile_first_window (m-tiles of `tile` rows), stride1, taps_swapped, pad_not_zeroed, pos_clamped,
      resid_twice, gelu_tanh"""
    N, M, K = c["N"], c["M"], c["K"]
    w = weights(I, dt)
    if c["form"] == "conv":
        B, T, c_in = c["B"], c["T"], c["c_in"]
        if fault == "taps_swapped":
            w = w.reshape(N, 3, c_in).transpose(0, 2, 1)
        xp = np.zeros((B, c["rows"] + 2, c_in))
        xp[:, 1:-1] = I.x
        sb, sr = _conv_sources(c, fault, tile)
        v, mag = np.zeros((B, T, N)), np.zeros((B, T, N))
        for j in range(3):
            xs = xp[sb[:, :, j], sr[:, :, j]]                                 # [B][T][c_in]
            v += xs @ w[:, :, j].T
            mag += np.abs(xs) @ np.abs(w[:, :, j]).T
            if fault == "pad_not_zeroed":                                     # pad weights of 1 meet PAD_FILL on every interior row
                interior = (sr[:, :, j] >= 1) & (sr[:, :, j] <= c["rows"])
                v += (interior * PAD_FILL * (c["c_pad"] - c_in))[:, :, None]
        v, mag = v.reshape(M, N), mag.reshape(M, N)
    else:
        v, mag = I.x @ w.T, np.abs(I.x) @ np.abs(w).T
    v = v + I.bias[None, :]
    n_add = 0 if exact else K + 16
    bound = n_add * F32 * (mag + np.abs(I.bias)[None, :])
    if c["epi"] == EPI_BIAS_RESID_F32:
        v = v + I.resid * (2.0 if fault == "resid_twice" else 1.0)
        bound = bound + n_add * F32 * np.abs(I.resid)
    if is_gelu(c):
        bound = GELU_SLOPE * bound + GELU_TERM * np.maximum(1.0, np.abs(v))
        v = gelu_tanh(v) if fault == "gelu_tanh" else gelu(v)
    if c["epi"] == EPI_GELU_POS_F32:
        _, t = window_rows(c)
        p = I.pos[np.minimum(np.arange(M), c["T"] - 1) if fault == "pos_clamped" else t]
        bound = bound + F32 * (np.abs(v) + np.abs(p))
        v = v + p
    if not out_is_f32(c):
        bound = bound + np.maximum(ULP[dt] * (np.abs(v) + bound), 2.0 ** -24 if dt == 1 else 0.0)
    return v + 0.0, bound


# ---- where the values go ------------------------------------------------------------------------------------------------------

def place_index(c, fault=None, tile=128):
    """[M][N] -> element of the output image that holds output (m, n).
    fault: out_row_t, tile_first_window_out (m-tiles of `tile` rows), batch_offset_dropped, head_pos_swapped, slab_wrong_d,
      map_ignored"""
    N, M = c["N"], c["M"]
    b, t = window_rows(c)
    n = np.arange(N)[None, :]
    if c["form"] == "xkv":
        d, H, TL = c["d_model"], c["H"], c["t_len"]
        if fault == "map_ignored":            # (window, position) from m / rows_per_batch, and a packed launch has rows_per_batch = M
            b, t = np.zeros(M, dtype=np.int64), np.arange(M)
        if fault == "slab_wrong_d":           # the slab as n / (N / 2L) with a d_model one head too large
            d = d + 64
        slab, rem = n // d, n % d
        h, dh = rem // 64, rem % 64
        w = slab * c["batch"] + (0 if fault == "batch_offset_dropped" else c["first"]) + b[:, None]
        if fault == "head_pos_swapped":
            return ((w * TL + t[:, None]) * H + h) * 64 + dh
        return ((w * H + h) * TL + t[:, None]) * 64 + dh
    shift = 0 if fault == "out_row_t" else row_shift(c)
    if fault == "tile_first_window_out":
        m = np.arange(M)
        b = (m // tile * tile) // c["T"]
        t = m - b * c["T"]
    return ((b * out_pitch(c) + shift + t)[:, None]) * N + n


def image_elems(c):
    if c["form"] == "xkv":
        return c["N"] // c["d_model"] * c["batch"] * c["H"] * c["t_len"] * 64
    return c["B"] * out_pitch(c) * c["N"]


def guard_elems(c):
    return GUARD_ROWS * (64 if c["form"] == "xkv" else c["N"])


def images(c, I=None):
    """the output buffer as the test pre-fills it (flat float64): SENTINEL everywhere, guard rows included; the rows a RESID line
    names hold the residual"""
    img = np.full(image_elems(c) + guard_elems(c), SENTINEL)
    if c["epi"] == EPI_BIAS_RESID_F32 and I is not None:
        img[place_index(c)] = I.resid
    return img


def place(c, img, v, fault=None, tile=128):
    """store v [M][N] where the contract stores it (in place); what it does not name is left alone"""
    img[place_index(c, fault, tile)] = v
    return img


# ---- fp32 emulation through the GEMM view (CPU tests) -----------------------------------------------------------------------------

def emulate(c, I, dt, rng):
    """what a kernel computes, as far as numpy can say it, from what the kernel is GIVEN: the A buffer of a_image() addressed by
    geometry(), the weights as the loader's kernels leave them (pad channels zero); fp32 products and sums, the 32-column
    k-blocks summed in a shuffled order -> the converted output [M][N]"""
    f = np.float32
    g = geometry(c)
    M, N, K = g["M"], g["N"], g["K"]
    a = a_image(c, I).reshape(-1)
    assert a.size == g["a_elems"]
    m = np.arange(M)
    start = (m // g["rows_per_batch"]) * g["a_batch_stride"] + (m % g["rows_per_batch"]) * g["lda"]
    A = a[start[:, None] + np.arange(K)[None, :]].astype(f)
    w16 = weights(I, dt)
    W = (repacked(c, w16).reshape(N, K) if c["form"] == "conv" else w16).astype(f)
    part = np.einsum("mbk,nbk->bmn", A.reshape(M, K // 32, 32), W.reshape(N, K // 32, 32)).astype(f)
    acc = np.zeros((M, N), dtype=f)
    for j in rng.permutation(K // 32):
        acc = acc + part[j]
    acc = acc + I.bias.astype(f)[None, :]
    if c["epi"] == EPI_BIAS_RESID_F32:
        acc = I.resid.astype(f) + acc
    if is_gelu(c):
        acc = gelu(acc.astype(np.float64)).astype(f)
    if c["epi"] == EPI_GELU_POS_F32:
        acc = acc + I.pos.astype(f)[m % g["rows_per_batch"]]
    out = acc.astype(np.float64)
    if out_is_f32(c):
        return out
    out[np.abs(out) < 1e-30] = 0.0            # round_T models bf16's normal range only; 1e-30 is far below every bound
    return round_T(out, dt)
