"""Inputs, float64 reference and error bounds for the decoder GEMM family (launch_dec_gemm, decode.hip) and the load-time
kernels in front of it (fold_ln, repack_tiled, tiled_rowsum), the embedding and the LayerNorm launch.  Plain numpy, no GPU.

A case is a dict (see case()): epilogue, operand form, M, N, K and what steers the work shape.  make() builds its inputs:

  exact  small integers, so that every product, partial sum and final sum is an integer (or a multiple of 1/2) far below 2^24:
         an fp32 result is then THE result whatever the summation order, and a 16-bit output is that value rounded once.
         ln / pn rows are x[m][k] = mu_m + c_m * s[m][k], s = +-1 with eight of each sign in every 16 columns: the fp32 sum,
         the mean (mu_m), the deviations (+-c_m) and every statistics tile (mu_m, 16 c_m^2) are exact, Chan's merge of equal
         means is exact, and (x - mean) * rstd = +-(1 - ~5e-6 / c^2) rounds to exactly +-1 in bf16 and f16 (c >= 1: with a
         smaller c the 1e-5 epsilon moves the f16 rounding).  gamma is a power of two and beta an integer: the fold is exact.
  real   Gaussian values rounded to the 16-bit type; gamma stays a power of two so that the folded weights are still exactly
         representable and the reference needs no model of the weights' rounding.

forward() is the reference, written from the definition  f(x) W'^T + b'  with  W' = W gamma, b' = b + W beta  and f = identity
or LayerNorm, in float64; it returns the value of every output element before its final conversion, and the bound on
|kernel - reference| next to it.  place() puts values where the epilogue stores them; everything else in an output image keeps
SENTINEL.  The fault-injection tests (test_dec_gemm_ref_cpu.py) edit this description through forward()'s and place()'s
`fault` argument, never a kernel.
"""
import math
import zlib

import numpy as np

from attn_needles import act_tiled_index, tiled_elems

QKV, BIAS_T, GELU_T, RESID, LOGITS = range(5)          # kernels.hpp DecEpilogue
PLAIN, LN, PN = range(3)                               # operand forms (ohw.h OHW_DG_FORM_*)
S1x1, S2x1, S1x2, S2x2, S4x2, S1x6 = range(6)          # kernels.hpp DecGemmShape
SHAPE_NAMES = ("1x1", "2x1", "1x2", "2x2", "4x2", "1x6")
EPI_NAMES = ("qkv", "bias_t", "gelu_t", "resid", "logits")
FORM_NAMES = ("plain", "ln", "pn")
SENTINEL = 77.0          # exact in f32, bf16 and f16
EPS = 1e-5               # the LayerNorm epsilon
GUARD_ROWS = 3
GUARD_TILE = 512         # elements behind a tiled image

# one ulp of the 16-bit type relative to the value (8 / 11 significand bits), and half of it (one rounding to nearest)
ULP = {0: 2.0 ** -8, 1: 2.0 ** -11}
HALF = {0: 2.0 ** -9, 1: 2.0 ** -12}
F32 = 2.0 ** -23         # a faithfully rounded fp32 operation errs by less than this, relative (twice the round-to-nearest 2^-24)


def case(epi, form, M, N, K, cu=0, shape=None, n_new=1, ld=None, ksplit=0, stat=False, n_past=None, n_ctx=None):
    """ld: row stride of BIAS_T / RESID / LOGITS outputs (default N); stat: the RESID producer (x16_out, stat_out);
    QKV: d_model = N / 3, n_head = d_model / 64, n_past [M / n_new], n_ctx"""
    c = dict(epi=epi, form=form, M=M, N=N, K=K, cu=cu, shape=shape, n_new=n_new, ld=N if ld is None else ld, ksplit=ksplit, stat=stat)
    if epi == QKV:
        c.update(d_model=N // 3, n_head=N // 192, n_past=list(n_past), n_ctx=n_ctx)
    return c


def case_name(c):
    return (f"{EPI_NAMES[c['epi']]}.{FORM_NAMES[c['form']]}" + (".ks%d" % c["ksplit"] if c["ksplit"] > 1 else "") + (".stat" if c["stat"] else "") +
            f"-M{c['M']}-N{c['N']}-K{c['K']}-cu{c['cu']}-n{c['n_new']}")


def out_is_f32(c):
    return c["epi"] in (RESID, LOGITS)


# ---- the 16-bit formats ---------------------------------------------------------------------------------------------------

def round_T(a, dt):
    """float64 -> the nearest bf16 (dt 0) / f16 (dt 1) value, ties to even, ONE rounding, as float64"""
    a = np.asarray(a, dtype=np.float64)
    if dt == 1:
        return a.astype(np.float16).astype(np.float64)
    m, e = np.frexp(a)                                  # a = m * 2^e, 0.5 <= |m| < 1: eight significand bits = multiples of 2^(e - 8)
    assert (np.abs(a[a != 0]) > 1e-30).all() and (np.abs(a) < 1e30).all()       # bf16's normal range is all that is modelled
    return np.ldexp(np.rint(np.ldexp(m, 8)), e - 8)


def bits_T(a, dt):
    """the raw 16-bit words of values that are exactly representable"""
    a = np.asarray(a, dtype=np.float64)
    if dt == 1:
        h = a.astype(np.float16)
        assert (h.astype(np.float64) == a).all()
        return h.view(np.uint16)
    f = a.astype(np.float32)
    w = f.view(np.uint32)
    assert (f.astype(np.float64) == a).all() and not (w & 0xffff).any()
    return (w >> 16).astype(np.uint16)


def weight_tiled_index(N, K):
    """repack_tiled (weights.hip): element (n, k) of T [ceil16(N) / 16][K / 32][64][8]: act_tiled_index with n in place of m"""
    return act_tiled_index(N, K)


# ---- statistics tiles -------------------------------------------------------------------------------------------------------

def tile_stats(x):
    """[M][K] -> [M][K / 16][2]: mean and sum of squared deviations of every 16 columns (float64)"""
    t = np.asarray(x, dtype=np.float64).reshape(x.shape[0], -1, 16)
    mean = t.mean(axis=2)
    return np.stack([mean, ((t - mean[:, :, None]) ** 2).sum(axis=2)], axis=2)


def merge_tiles(tiles, order=None, dtype=np.float64):
    """Chan's update over the tiles of ONE row ([n][2]) in `order` (default 0 .. n - 1; an index may repeat: the fault) ->
    (count, mean, m2) in `dtype` arithmetic"""
    f = dtype
    cnt, mean, m2 = f(0), f(0), f(0)
    for j in (range(len(tiles)) if order is None else order):
        nn = f(cnt + f(16))
        delta = f(f(tiles[j][0]) - mean)
        mean = f(mean + f(delta * f(f(16) / nn)))
        m2 = f(m2 + f(f(tiles[j][1]) + f(f(delta * delta) * f(f(cnt * f(16)) / nn))))
        cnt = nn
    return cnt, mean, m2


def stat_bounds(x16cols):
    """bounds on the fp32 (mean, m2) of 16 values [..., 16] as embed_kernel / the RESID producer compute them.
    mean: at most 15 additions, each within 2^-24 of a partial sum <= sum |x|, then an exact multiplication by 1/16:
      |mean' - mean| <= 15 * 2^-24 * sum|x| / 16 < 2^-24 * sum|x| =: e.
    m2: the deviations are d'_c = (x_c - mean')(1 + 2^-24); sum_c (x_c - mean) = 0, so the error of the mean enters only as
      16 e^2; a square is three roundings, the sum of 16 of them at most 15 more: relative 18 * 2^-24, stated as 24 * 2^-24."""
    a = np.abs(np.asarray(x16cols, dtype=np.float64))
    e = 2.0 ** -24 * a.sum(axis=-1)
    t = np.asarray(x16cols, dtype=np.float64)
    m2 = ((t - t.mean(axis=-1, keepdims=True)) ** 2).sum(axis=-1)
    return e, 24 * 2.0 ** -24 * m2 + 16 * e * e + 1e-37


# ---- inputs -------------------------------------------------------------------------------------------------------------------

class Inputs:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _rng(c, kind, dt, seed):
    # keyed by what shapes the data, not by what steers the kernel choice (cu, ksplit): cases that differ only there share inputs
    key = (c["epi"], c["form"], c["M"], c["N"], c["K"], c["n_new"])
    return np.random.default_rng([zlib.crc32(repr(key).encode()), int(kind == "real"), dt, seed])


def _signs(rng, M, K):
    """+-1 [M][K], eight of each sign in every 16 columns"""
    base = np.array([1.0] * 8 + [-1.0] * 8)
    return np.stack([np.concatenate([rng.permutation(base) for _ in range(K // 16)]) for _ in range(M)])


def make(c, kind, dt, seed=0):
    """-> Inputs: w [N][K], bias [N], gamma / beta [K] or None (ln and pn forms have them), x [M][K] (ln: fp32 values, else
    values of the 16-bit type), stat f32 [M][K / 16][2] (pn), resid [M][N] (RESID).  All float64 arrays of exactly representable
    values"""
    rng = _rng(c, kind, dt, seed)
    M, N, K, form = c["M"], c["N"], c["K"], c["form"]
    normed = form in (LN, PN)
    I = Inputs(gamma=None, beta=None, stat=None, resid=None, mu=None, cdev=None)
    if kind == "exact":
        I.w = rng.integers(-4, 5, size=(N, K)).astype(np.float64)
        if form == PN:
            # the pn epilogue multiplies by an INEXACT rstd = (1 - ~5e-6 / c^2) / c: out = h (1 - ~5e-6 / c^2) + b' with an integer
            # h.  The 16-bit output is a decided word only while h + b' is a value the type holds and the shift 5e-6 |h| / c^2
            # stays far inside the rounding interval around it (pn_exact_margin).  About 48 non-zero weights of size <= 2 per
            # row (gamma 1 or 2: integers) keep h near +-20, c >= 2 quarters the shift ...
            I.w = np.where(rng.random((N, K)) < min(1.0, 48.0 / K), rng.integers(-2, 3, size=(N, K)), 0).astype(np.float64)
        I.bias = rng.integers(-4, 5, size=N).astype(np.float64)
        if form == PN:
            I.bias = I.bias + 0.5        # ... and an integer + 1/2 is never near zero, where the rounding intervals shrink
        if normed:
            I.gamma = 2.0 ** (rng.integers(-1, 2, size=K) if form == LN else rng.integers(0, 2, size=K))
            I.beta = rng.integers(-2, 3, size=K).astype(np.float64)
            if form == PN:
                I.beta = np.where(rng.random(K) < min(1.0, 8.0 / K), np.sign(I.beta), 0.0)
            I.mu = ((np.arange(M) * 5 + int(rng.integers(0, 17))) % 17 - 8).astype(np.float64)      # neighbours differ
            I.cdev = 2.0 ** rng.integers(1 if form == PN else 0, 3, size=M)
            I.x = I.mu[:, None] + I.cdev[:, None] * _signs(rng, M, K)
        else:
            I.x = rng.integers(-4, 5, size=(M, K)).astype(np.float64)
        if c["epi"] == RESID:
            I.resid = rng.integers(-4, 5, size=(M, N)).astype(np.float64)
    else:
        I.w = round_T(rng.standard_normal((N, K)) / math.sqrt(K), dt)
        I.bias = round_T(rng.standard_normal(N), dt)
        if normed:
            I.gamma = 2.0 ** rng.integers(-1, 2, size=K)
            I.beta = round_T(0.5 * rng.standard_normal(K), dt)
            scale = rng.uniform(0.5, 3.0, size=M)
            I.x = round_T(scale[:, None] * (rng.standard_normal((M, K)) + rng.standard_normal(M)[:, None]), dt)
        else:
            I.x = round_T(rng.standard_normal((M, K)), dt)
        if c["epi"] == RESID:
            I.resid = round_T(rng.standard_normal((M, N)), dt)
    if form == PN:
        I.stat = tile_stats(I.x).astype(np.float32)
    return I


# ---- the reference --------------------------------------------------------------------------------------------------------------

def gelu(v):
    return 0.5 * v * (1.0 + np.vectorize(math.erf)(v / math.sqrt(2.0)))


def gelu_tanh(v):
    return 0.5 * v * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v ** 3)))


GELU_TERM = 2e-6         # |gelu_erf_fp32(v) - gelu(v)| <= 2e-6 * max(1, |v|): 1.5e-7 of the A&S 7.1.26 erf, plus about a dozen fp32
                         # roundings (rcp, five Horner steps, exp2, three products, two sums) of quantities <= max(1, |v|): 12 * 2^-23 = 1.4e-6
GELU_SLOPE = 1.13        # max |gelu'| = 1.1289: what an error of the pre-activation becomes


def folded(I):
    """(W', b', sum_k |beta_k w_k| + |b|): launch_fold_ln, exact in float64"""
    W = I.w if I.gamma is None else I.w * I.gamma[None, :]
    b = np.zeros(I.w.shape[0]) if I.bias is None else I.bias.copy()
    mag = np.abs(b)
    if I.beta is not None:
        b = b + I.w @ I.beta
        mag = mag + np.abs(I.w) @ np.abs(I.beta)
    return W, b, mag


def forward(c, I, dt, round_y=False, fault=None, kb=0, dup_tile=0, exact=False):
    """-> (v [M][N], bound [M][N]): every output element before its final conversion (fp32, or the 16-bit type), float64, and
    the bound on |kernel - v| after that conversion.

    round_y (the exact inputs of the ln form): the kernel rounds the normalised row to the 16-bit type before the product; on
    the exact inputs that is +-1 exactly and the output is decided bit for bit.  On real inputs the bound carries that rounding.

    Bound, per element, every term from the number formats:
      fp32 accumulation  (K + 16) * 2^-23 * (sum_k |y_k w'_k| + |b| + sum_k |beta_k w_k| + |resid|): at most K + 16 additions
                         (K products into the accumulators, 8 partial sums, bias, residual, the fold's own tree), each
                         faithfully rounded on a partial sum no larger than the sum of the magnitudes
      ln                 + 2^-9 / 2^-12 * sum_k |y_k w'_k|: y is rounded once to the 16-bit type before the product
      pn                 the accumulation term sits on rstd * (sum_k |x_k w'_k| + |mean * wsum|): the kernel forms both and
                         subtracts (the statistics' own handful of fp32 roundings ride in the K + 16 count)
      GELU               1.13 * (the above) + 2e-6 * max(1, |v|)   (GELU_SLOPE, GELU_TERM)
      16-bit output      + one ulp of the type at |v| (2^-8 / 2^-11 relative; f16: at least its subnormal step 2^-24)
    exact (the exact inputs, where only the GELU lines need a bound): no accumulation term - the sums are exact - but for the two
      roundings of the pn epilogue (the product with rstd, the bias).
    fault: drop_kblock / twice_kblock (k-block kb), swap_ntiles (tiles 0 and 1), skip_bias_last_tile, mean_next_row,
      stat_tile_twice (tile dup_tile), gelu_tanh, resid_twice"""
    M, N, K, form, epi = c["M"], c["N"], c["K"], c["form"], c["epi"]
    W, b, mag_b = folded(I)
    x = I.x
    if form in (LN, PN):
        mean = x.mean(axis=1)
        var = ((x - mean[:, None]) ** 2).mean(axis=1)
        if fault == "stat_tile_twice":
            tiles = tile_stats(x)
            order = list(range(K // 16)) + [dup_tile]
            merged = [merge_tiles(tiles[m], order) for m in range(M)]
            mean = np.array([t[1] for t in merged])
            var = np.array([t[2] for t in merged]) / K
        if fault == "mean_next_row":
            mean = np.roll(mean, -1)
        rstd = 1.0 / np.sqrt(var + EPS)
        y = (x - mean[:, None]) * rstd[:, None]
        if round_y and form == LN:
            y = round_T(y, dt)
    else:
        y = x
    yk = y
    if fault in ("drop_kblock", "twice_kblock"):
        yk = y.copy()
        yk[:, kb * 32:(kb + 1) * 32] *= 0.0 if fault == "drop_kblock" else 2.0
    v = yk @ W.T
    if form == PN:
        mag = rstd[:, None] * (np.abs(x) @ np.abs(W).T + np.abs(mean[:, None] * W.sum(axis=1)[None, :]))
    else:
        mag = np.abs(y) @ np.abs(W).T
    if fault == "swap_ntiles":
        v[:, 0:16], v[:, 16:32] = v[:, 16:32].copy(), v[:, 0:16].copy()
    bb = b.copy()
    if fault == "skip_bias_last_tile":
        bb[(N - 1) // 16 * 16:] = 0.0
    v = v + bb[None, :]
    n_add = (2 if form == PN else 0) if exact else K + 16
    bound = n_add * F32 * (mag + mag_b[None, :])
    if form == LN and not round_y:
        bound = bound + HALF[dt] * mag
    if epi == RESID:
        v = v + I.resid * (2.0 if fault == "resid_twice" else 1.0)
        bound = bound + n_add * F32 * np.abs(I.resid)
    if epi == GELU_T:
        bound = GELU_SLOPE * bound + GELU_TERM * np.maximum(1.0, np.abs(v))
        v = gelu_tanh(v) if fault == "gelu_tanh" else gelu(v)
    if not out_is_f32(c):
        # rounding to nearest moves a value by at most half the spacing, 2^-8 / 2^-11 of it at the bottom of a binade; the value
        # that is rounded is the kernel's, within `bound` of v
        bound = bound + np.maximum(ULP[dt] * (np.abs(v) + bound), 2.0 ** -24 if dt == 1 else 0.0)
    return v + 0.0, bound


def pn_exact_margin(I, v, dt):
    """the exact inputs of the pn form: v = h (1 - ~5e-6 / c^2) + b' (forward()).  True where the nominal value n = h + b', an
    integer + 1/2, is held by the 16-bit type and v lies within a quarter of the distance from n to its rounding boundary
    (2^-9 / 2^-12 of |n| at least): the kernel's own fp32 roundings (rsqrt, one product, one sum: 3e-7 relative) cannot change
    the word then"""
    n = np.rint(v - 0.5) + 0.5
    return (round_T(n, dt) == n) & (np.abs(v - n) <= 0.25 * HALF[dt] * np.abs(n))


# ---- where the values go ------------------------------------------------------------------------------------------------------

def images(c, I=None):
    """name -> the output buffers as the test pre-fills them (float64; SENTINEL everywhere, the RESID rows hold the residual)"""
    M, N, epi = c["M"], c["N"], c["epi"]
    if epi == QKV:
        d, H, B = c["d_model"], c["n_head"], M // c["n_new"]
        return {"out": np.full((M + GUARD_ROWS, d), SENTINEL), "k_cache": np.full((B + 1, H, c["n_ctx"], 64), SENTINEL),
                "v_cache": np.full((B + 1, H, c["n_ctx"], 64), SENTINEL)}
    if epi == GELU_T:
        return {"out": np.full(tiled_elems(M, N) + GUARD_TILE, SENTINEL)}
    if epi == LOGITS:
        return {"out": np.full((M // c["n_new"] + GUARD_ROWS, c["ld"]), SENTINEL)}
    img = {"out": np.full((M + GUARD_ROWS, c["ld"]), SENTINEL)}
    if epi == RESID and I is not None:
        img["out"][:M, :N] = I.resid
    if c["stat"]:
        img["x16_out"] = np.full(tiled_elems(M, N) + GUARD_TILE, SENTINEL)
        img["stat_out"] = np.full((M + GUARD_ROWS, N // 16, 2), SENTINEL)
    return img


def place(c, img, v, fault=None):
    """store v [M][N] into the images where the epilogue stores it (in place); what the contract does not name is left alone.
    fault: kv_pos_plus1, logits_row_before (the row n_new - 2 of a window)"""
    M, N, epi = c["M"], c["N"], c["epi"]
    if epi == QKV:
        d, H, n_new, C = c["d_model"], c["n_head"], c["n_new"], c["n_ctx"]
        img["out"][:M] = v[:, :d]
        for m in range(M):
            b, i = divmod(m, n_new)
            pos = c["n_past"][b] + i + (1 if fault == "kv_pos_plus1" else 0)
            if pos < C:
                img["k_cache"][b, :, pos, :] = v[m, d:2 * d].reshape(H, 64)
                img["v_cache"][b, :, pos, :] = v[m, 2 * d:].reshape(H, 64)
    elif epi == GELU_T:
        img["out"][act_tiled_index(M, N)] = v
    elif epi == LOGITS:
        n_new = c["n_new"]
        pick = n_new - 2 if fault == "logits_row_before" else n_new - 1
        img["out"][:M // n_new, :N] = v[pick::n_new]
    else:
        img["out"][:M, :N] = v
    return img


def producer_expect(c, out_f32, dt):
    """the RESID producer's x16_out and stat_out from the fp32 rows it stored ([M][N], as float64): the 16-bit copy is those
    values rounded once; the statistics within stat_bounds -> (x16 image, stat [M][N / 16][2], stat bound [M][N / 16][2])"""
    M, N = c["M"], c["N"]
    x16 = np.full(tiled_elems(M, N) + GUARD_TILE, SENTINEL)
    x16[act_tiled_index(M, N)] = round_T(out_f32, dt)
    e, q = stat_bounds(out_f32.reshape(M, N // 16, 16))
    return x16, tile_stats(out_f32), np.stack([e, q], axis=2)


# ---- fp32 emulation (CPU tests: the reference stays inside its own bounds) ------------------------------------------------------

def emulate(c, I, dt, rng):
    """what a kernel computes, as far as numpy can say it: fp32 products and sums, the k-blocks summed in a shuffled order, the
    16-bit roundings where the kernel has them, fp32 statistics (pn: Chan's merge of the fp32 tiles) -> the converted output"""
    f = np.float32
    M, N, K, form, epi = c["M"], c["N"], c["K"], c["form"], c["epi"]
    W, b, _ = folded(I)
    W32, b32 = W.astype(f), b.astype(f)           # real inputs: the fold's fp32 sum differs from this by what the bound's fold term covers
    x = I.x.astype(f)
    if form == LN:
        mean = (x.sum(axis=1, dtype=f) / f(K)).astype(f)
        dev = x - mean[:, None]
        rstd = (f(1) / np.sqrt((dev * dev).sum(axis=1, dtype=f) / f(K) + f(EPS))).astype(f)
        y = round_T((dev * rstd[:, None]).astype(np.float64), dt).astype(f)
    else:
        y = x
    part = np.einsum("mbk,nbk->bmn", y.reshape(M, K // 32, 32), W32.reshape(N, K // 32, 32)).astype(f)
    acc = np.zeros((M, N), dtype=f)
    for j in rng.permutation(K // 32):
        acc = acc + part[j]
    if form == PN:
        merged = [merge_tiles(I.stat[m], dtype=np.float32) for m in range(M)]
        mean = np.array([t[1] for t in merged], dtype=f)
        rstd = (f(1) / np.sqrt(np.array([t[2] for t in merged], dtype=f) / f(K) + f(EPS))).astype(f)
        acc = rstd[:, None] * (acc - mean[:, None] * W32.sum(axis=1, dtype=f)[None, :])
    acc = acc + b32[None, :]
    if epi == RESID:
        acc = I.resid.astype(f) + acc
    if epi == GELU_T:
        acc = gelu(acc.astype(np.float64)).astype(f)
    return acc.astype(np.float64) if out_is_f32(c) else round_T(acc.astype(np.float64), dt)


def layernorm_ref(x, gamma, beta, dt):
    """LayerNorm launch (misc.hip): -> (y float64 before the conversion, bound).  fp32 term: the mean and the variance are sums
    of d terms (at most d / 4 + 8 roundings each on the kernel's tree, stated as d), normalisation and affine part six more:
    (d + 6) * 2^-23 * (|y_hat gamma| + |beta|) covers them with y_hat = (x - mean) * rstd; plus one ulp of the 16-bit type"""
    mean = x.mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(((x - mean) ** 2).mean(axis=1, keepdims=True) + EPS)
    yh = (x - mean) * rstd
    y = yh * gamma[None, :] + beta[None, :]
    # a rounding error of the mean is relative to |x|, not to the deviation: rows with an offset feel it through |mean| * rstd
    mag = (np.abs(yh) + np.abs(mean) * rstd) * np.abs(gamma)[None, :] + np.abs(beta)[None, :]
    b32 = (x.shape[1] + 6) * F32 * mag
    return y, b32 + np.maximum(ULP[dt] * (np.abs(y) + b32), 2.0 ** -24 if dt == 1 else 0.0)
