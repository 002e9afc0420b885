"""The encoder GEMM kernels (gemm.hip 128x128, gemm256.hip 256x256, gemm_small.hip 64x64) in the forms run_encode launches them -
conv1 and conv2 over overlapping rows of a padded image, the head-major cross-K/V store with batch / batch_offset and the
packed-row map, the row-major epilogues under a per-window row remap - against the float64 reference of tests/enc_gemm_ref.py,
through ohw_dbg_enc_gemm on caller data.  The weights go in as fp32 and are prepared by the loader's own convert_rows /
repack_conv.

Every table line runs under each of the three kernels, in both dtypes, on the exact inputs (raw words must equal the
reference's) and on the real ones (every element within its derived bound; the worst error / bound per form and kernel is
printed).  Output images are pre-filled with a sentinel and carry guard rows: every element the contract does not name must
still hold the sentinel afterwards.

GELU lines on the exact inputs: the pre-activation is exact but the GELU is not, so they are held to the GELU term of the bound
alone (2e-6 max(1, |v|), conv2's one fp32 addition of pos, one ulp of a 16-bit output) instead of word equality.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import enc_gemm_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LINES = list(R.TABLE)
KERNELS = [R.K128, R.SMALL, R.K256]
WORST = {}       # (line, kernel) -> worst error / bound on the real inputs, over both dtypes
RUNS = {}        # (line, kernel, kind, dt) -> the raw words of the whole output image


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


def _words(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu().numpy().view(np.uint16 if t.element_size() == 2 else np.uint32)


def _want_words(a, dt, f32):
    return np.asarray(a, dtype=np.float32).view(np.uint32) if f32 else R.bits_T(R.round_T(a, dt), dt)


@functools.lru_cache(maxsize=None)
def reference(name, kind, dt):
    """computed once per (line, input kind, dtype) and shared by the kernels: the inputs, the output image as the test pre-fills
    it, the expected image, and the image of bounds (zero wherever the sentinel must stay)"""
    c = R.TABLE[name]
    I = R.make(c, kind, dt)
    v, bound = R.forward(c, I, dt, exact=kind == "exact")
    before = R.images(c, I)
    want = R.place(c, before.copy(), v)
    lim = R.place(c, np.zeros(before.size), bound)
    for a in (before, want, lim):
        a.setflags(write=False)
    return I, before, want, lim


def launch(E, name, kernel, kind, dt):
    """one ohw_dbg_enc_gemm of a table line -> the whole output image (device tensor, guard rows included)"""
    c = R.TABLE[name]
    g = R.geometry(c)
    I, before, _, _ = reference(name, kind, dt)
    td = _td(dt)
    otd = torch.float32 if R.out_is_f32(c) else td
    held = dict(a=_dev(R.a_image(c, I).reshape(-1), td), w=_dev(I.w.reshape(-1)), bias=_dev(I.bias), pos=_dev(I.pos))
    out = _dev(before.copy(), otd)           # the shared image stays read-only
    assert held["a"].numel() == g["a_elems"]
    io = E.DbgEncGemmIO(dtype=dt, epilogue=c["epi"], kernel=kernel, conv_cin=g["conv_cin"], M=g["M"], N=g["N"], K=g["K"], lda=g["lda"],
                        a_batch_stride=g["a_batch_stride"], rows_per_batch=g["rows_per_batch"], ldc=g["ldc"], c_batch_stride=g["c_batch_stride"],
                        d_model=g["d_model"], n_head=g["n_head"], t_len=g["t_len"], batch=g["batch"], batch_offset=g["batch_offset"],
                        a=_ptr(held["a"]), a_elems=g["a_elems"], w=_ptr(held["w"]), bias=_ptr(held["bias"]), pos=_ptr(held["pos"]),
                        out=out.data_ptr() + g["out_offset"] * out.element_size(), out_elems=R.image_elems(c) - g["out_offset"])
    if c["form"] == "xkv" and c["packed"]:
        rmap = np.ascontiguousarray(R.row_map(c), dtype=np.int32)
        io.c_row_map = E._ip(rmap)
    rc = E.lib().ohw_dbg_enc_gemm(C.byref(io), torch.cuda.current_stream().cuda_stream)
    if rc not in (0, E.OHW_E_INVALID_ARG):
        pytest.exit(f"{name} {R.KERNEL_NAMES[kernel]}: the device reported an error ({E.last_error()}): nothing more is launched", 3)
    assert rc == 0, (name, R.KERNEL_NAMES[kernel], E.last_error())
    torch.cuda.synchronize()
    return out


def words_of(E, name, kernel, kind, dt):
    key = (name, kernel, kind, dt)
    if key not in RUNS:
        RUNS[key] = _words(launch(E, name, kernel, kind, dt))
    return RUNS[key]


def check(name, kind, dt, out, tag):
    """the output image against the reference: words on the exact inputs, bounds on the real ones, the sentinel everywhere else"""
    c = R.TABLE[name]
    _, _, want, lim = reference(name, kind, dt)
    f32 = R.out_is_f32(c)
    if kind == "exact" and not R.is_gelu(c):
        bad = np.argwhere(_words(out) != _want_words(want, dt, f32))
        assert len(bad) == 0, (tag, len(bad), bad[:4].tolist())
        return 0.0
    got = out.double().cpu().numpy()
    err = np.abs(got - want)
    ok = err <= lim                              # a NaN fails; where the contract names nothing the bound is 0: the sentinel
    assert ok.all(), (tag, int((~ok).sum()), np.argwhere(~ok)[:4].tolist(), float(np.nanmax(err / np.maximum(lim, 1e-300))))
    named = lim > 0
    return float((err[named] / lim[named]).max())


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("kernel", KERNELS, ids=[R.KERNEL_NAMES[k] for k in KERNELS])
@pytest.mark.parametrize("name", LINES)
def test_table_line(E, name, kernel, kind, dt):
    assert R.TABLE[name]["N"] % R.KERNEL_N[kernel] == 0
    out = launch(E, name, kernel, kind, dt)
    RUNS[(name, kernel, kind, dt)] = _words(out)
    worst = check(name, kind, dt, out, f"{name} {R.KERNEL_NAMES[kernel]} {kind} dt {dt}")
    if kind == "real":
        key = (name, R.KERNEL_NAMES[kernel])
        WORST[key] = max(WORST.get(key, 0.0), worst)
        print(f"enc_gemm {name} {key[1]} {'bf16' if dt == 0 else 'f16'}: worst error / bound {worst:.3f}; line and kernel so far {WORST[key]:.3f}")


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("name", LINES)
def test_small_and_auto_give_the_128_kernels_words(E, name, dt):
    """gemm_small.hip claims the bits of gemm.hip (the same accumulation order per element); launch_gemm's own pick on these shapes
    is the 128x128 kernel.  Nothing of the kind is claimed for the 256x256 kernel"""
    k128 = words_of(E, name, R.K128, "real", dt)
    small = words_of(E, name, R.SMALL, "real", dt)
    auto = words_of(E, name, R.AUTO, "real", dt)
    assert (small == k128).all(), (name, int((small != k128).sum()))
    assert (auto == k128).all(), (name, int((auto != k128).sum()))


def _refused(E, rc, word):
    assert rc == E.OHW_E_INVALID_ARG, rc
    assert word in E.last_error(), E.last_error()


def test_rejections_launch_nothing(E):
    """every refusal comes before any device work: the buffer behind every pointer is far too small for the stated sizes and is
    still whole afterwards"""
    buf = torch.full((256,), R.SENTINEL, device="cuda")
    p = buf.data_ptr()
    assert p % 16 == 0
    rmap = np.zeros(19, dtype=np.int32)

    def call(**kw):
        a = dict(dtype=0, epilogue=R.EPI_BIAS_T, kernel=R.K128, conv_cin=0, M=19, N=256, K=64, lda=64, a_batch_stride=0, rows_per_batch=19, ldc=256,
                 c_batch_stride=0, a=p, a_elems=19 * 64, w=p, bias=p, out=p, out_elems=19 * 256)
        a.update(kw)
        return E.lib().ohw_dbg_enc_gemm(C.byref(E.DbgEncGemmIO(**a)), None)

    xkv = dict(epilogue=R.EPI_CROSSKV_T, d_model=128, n_head=2, t_len=10, batch=2, batch_offset=1, M=5, rows_per_batch=5, a_elems=5 * 64,
               out_elems=2 * 2 * 2 * 10 * 64, ldc=0)
    # the four the table's contract names
    _refused(E, call(c_row_map=E._ip(rmap)), "row map goes with the cross-K/V")
    rmap[4] = 10
    _refused(E, call(**dict(xkv, c_row_map=E._ip(rmap))), "c_row_map[4] = 10")
    rmap[4] = -1
    _refused(E, call(**dict(xkv, c_row_map=E._ip(rmap))), "c_row_map[4] = -1")
    rmap[4] = 0
    _refused(E, call(a_elems=19 * 64 - 1), "past a_elems")
    _refused(E, call(kernel=R.K256, N=384, ldc=384, out_elems=19 * 384), "multiple of 256")
    # and the rest of the ranges
    _refused(E, call(M=300, rows_per_batch=100, lda=64, a_batch_stride=102 * 64, K=192, a_elems=3 * 102 * 64 - 1, out_elems=1 << 20), "past a_elems")
    _refused(E, call(out_elems=19 * 256 - 1), "past out_elems")
    _refused(E, call(M=38, a_elems=38 * 64, c_batch_stride=18 * 256, out_elems=1 << 20), "overlap")
    _refused(E, call(ldc=248), "ldc")
    _refused(E, call(ldc=260, out_elems=1 << 20), "multiples of 16 bytes")
    _refused(E, call(K=96, a_elems=1 << 20), "multiple of 64")
    _refused(E, call(lda=60), "multiples of 8")
    _refused(E, call(a=p + 2), "16-byte aligned")
    _refused(E, call(kernel=R.K128, N=192, ldc=192), "multiple of 128")
    _refused(E, call(kernel=R.SMALL, N=96, ldc=96), "multiple of 64")
    _refused(E, call(epilogue=6), "epilogue")
    _refused(E, call(kernel=4), "kernel")
    _refused(E, call(epilogue=R.EPI_GELU_POS_F32, pos=None), "needs pos")
    _refused(E, call(conv_cin=40), "conv weights")
    _refused(E, call(**dict(xkv, batch_offset=2)), "batch_offset")
    _refused(E, call(**dict(xkv, M=10, a_elems=10 * 64)), "exceed batch")
    _refused(E, call(**dict(xkv, M=11, rows_per_batch=11, a_elems=11 * 64)), "exceed t_len")
    _refused(E, call(**dict(xkv, n_head=3)), "d_model")
    _refused(E, call(**dict(xkv, out_elems=2 * 2 * 2 * 10 * 64 - 1)), "out_elems")
    torch.cuda.synchronize()
    assert (buf == R.SENTINEL).all()
