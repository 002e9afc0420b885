"""The prefill's cross-attention kernel (cross_attn_chunk_kernel, 8 query rows per window, both products on the MFMA units)
against the float64 reference of tests/attn_needles.py, through ohw_dbg_cross_attn_chunk: one key, or an exactly known pair,
decides every output, and every key past a window's length is poison.  Outputs are pre-filled with a sentinel that a finished
window's rows and the rows no window owns must keep.

Tolerance: attn_needles.TOL, unchanged (the kernel rounds P to 16 bits before P.V, as the encoder kernel does).  Every case
prints its worst error in tolerances.
"""
import numpy as np
import pytest

import attn_needles as A

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# decode.hip: XAC_KB keys per wave and block, 4 waves: the workgroup advances XAC_WG_KEYS keys per round
XAC_KB = 32
XAC_WG_KEYS = 4 * XAC_KB
# both sides of every block edge up to two blocks, of the wave's block and of the workgroup's round; then the sizes the issue names
EDGES = sorted({k * u + o for u in (XAC_KB, XAC_WG_KEYS) for k in (1, 2) for o in (-1, 0, 1)})
T_LENS = sorted(set(EDGES) | {1, 8, 250, 1500})
H = 2
WORST = {}


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from openhush_amd import engine
    engine.lib()
    return engine


def _td(dt):
    return torch.bfloat16 if dt == 0 else torch.float16


def _dev(a, td):
    return torch.from_numpy(np.array(a)).to(device="cuda", dtype=td)


_cases = {}


def _case(pattern, W, t_len, lens=None):
    key = (pattern, W, t_len, None if lens is None else tuple(lens))
    if key not in _cases:
        c = A.cross_case([ord(ch) for ch in f"chunk{pattern}{W}_{t_len}"], pattern, 8 * W, 8, t_len, lens=lens)
        ref = A.reference(c)
        for a in (c.q, c.K, c.V, ref):
            a.setflags(write=False)
        _cases[key] = (c, ref)
    return _cases[key]


def _run(E, c, dt, W, t_len, lens=None, done=None):
    td = _td(dt)
    M, d = 8 * W, 64 * H
    q, xk, xv = _dev(c.q.reshape(M, d), td), _dev(c.K, td), _dev(c.V, td)
    out = torch.full((A.tiled_elems(M, d),), A.SENTINEL, device="cuda", dtype=td)
    E.State.dbg_cross_attn_chunk(dt, q.data_ptr(), xk.data_ptr(), xv.data_ptr(), out.data_ptr(), W, H, t_len, win_len=lens, done=done,
                                 stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    idx = torch.from_numpy(A.act_tiled_index(M, d)).cuda()
    rest = torch.ones(out.numel(), dtype=torch.bool, device="cuda")
    rest[idx.reshape(-1)] = False
    return out[idx].double().cpu().numpy(), out[rest]


def _report(name, pattern, dt, err):
    key = "bf16" if dt == 0 else "f16"
    WORST[key] = max(WORST.get(key, 0.0), err)
    print(f"needles chunk {name} {pattern} {key}: worst error {err:.3e} = {err / A.TOL[dt]:.3f} tol; family so far "
          f"{WORST[key]:.3e} = {WORST[key] / A.TOL[dt]:.3f} tol")


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("pattern", A.PATTERNS)
@pytest.mark.parametrize("t_len", T_LENS)
def test_chunk_needles_uniform(E, t_len, pattern, dt):
    W = 3 if t_len <= 300 else 1          # 3 windows: an odd row count, the last activation tile half used
    c, ref = _case(pattern, W, t_len)
    got, rest = _run(E, c, dt, W, t_len)
    err = A.worst_error(got, ref)
    _report(f"t{t_len}", pattern, dt, err)
    assert err <= A.TOL[dt]
    assert (rest == A.SENTINEL).all()     # nothing past row 8 W - 1 of the last tile


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("pattern", A.PATTERNS)
def test_chunk_needles_window_lengths(E, pattern, dt):
    """per-window lengths under the envelope 250: the slab stride stays 250, the keys past a length are poison"""
    W = len(A.XA_LENS)
    c, ref = _case(pattern, W, 250, A.XA_LENS)
    got, rest = _run(E, c, dt, W, 250, lens=A.XA_LENS)
    err = A.worst_error(got, ref)
    _report("var", pattern, dt, err)
    assert err <= A.TOL[dt]
    assert (rest == A.SENTINEL).all()


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("pattern", A.PATTERNS)
@pytest.mark.parametrize("lens", [None, A.XA_LENS])
def test_chunk_needles_done_window_keeps_sentinel(E, lens, pattern, dt):
    W = len(A.XA_LENS)
    done = np.array([0, 0, 1, 0], dtype=np.int32)
    c, ref = _case(pattern, W, 250, lens)
    got, rest = _run(E, c, dt, W, 250, lens=lens, done=done)
    live = done[c.window] == 0
    err = A.worst_error(got[live], ref[live])
    _report("done" + ("_var" if lens else ""), pattern, dt, err)
    assert err <= A.TOL[dt]
    assert (got[~live] == A.SENTINEL).all()
    assert (rest == A.SENTINEL).all()


def test_chunk_entry_refuses_bad_arguments(E):
    """every refusal comes before any device work: the pointers are never dereferenced"""
    buf = torch.zeros(64, device="cuda", dtype=torch.bfloat16)
    p = buf.data_ptr()

    def refused(word, **kw):
        a = dict(windows=4, t_len=250, win_len=None)
        a.update(kw)
        with pytest.raises(E.WhisperError) as ei:
            E.State.dbg_cross_attn_chunk(0, p, p, p, p, a["windows"], 2, a["t_len"], win_len=a["win_len"])
        assert ei.value.code == E.OHW_E_INVALID_ARG and word in str(ei.value), str(ei.value)
    refused("below 1", windows=0)
    refused("below 1", t_len=0)
    refused("win_len[1] = 0", win_len=[250, 0, 1, 1])
    refused("win_len[1] = 251", win_len=[250, 251, 1, 1])
