"""The prefill's cross-attention kernel at 16 query rows per window (cross_attn_chunk_kernel<T, 16, VAR>, the 16-position chunks
of ohw_state_set_prefill_chunk) against the float64 reference of tests/attn_needles.py, through ohw_dbg_cross_attn_chunk_n: one
key, or an exactly known pair, decides every output, and every key past a window's length is poison.  Outputs are pre-filled
with a sentinel that a finished window's rows keep.

Tolerance: attn_needles.TOL, as in test_gpu_prefill_needles.py (the kernel is the same arithmetic per query column).
"""
import numpy as np
import pytest

import attn_needles as A

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NQ = 16
H = 2
W = 2
T_LENS = [1, 31, 32, 33, 129, 200]         # one key; a ragged last 32-key block; waves without a block (under 4 blocks)


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from openhush_amd import engine
    assert hasattr(engine.lib(), "ohw_dbg_cross_attn_chunk_n")
    return engine


def _td(dt):
    return torch.bfloat16 if dt == 0 else torch.float16


def _dev(a, td):
    return torch.from_numpy(np.array(a)).to(device="cuda", dtype=td)


_cases = {}


def _case(pattern, n_win, t_len, lens=None, tag=""):
    key = (pattern, n_win, t_len, None if lens is None else tuple(lens), tag)
    if key not in _cases:
        c = A.cross_case([ord(ch) for ch in f"chunk16{pattern}{n_win}_{t_len}{tag}"], pattern, NQ * n_win, NQ, t_len, lens=lens)
        ref = A.reference(c)
        for a in (c.q, c.K, c.V, ref):
            a.setflags(write=False)
        _cases[key] = (c, ref)
    return _cases[key]


def _run(E, c, dt, n_win, t_len, lens=None, done=None, n_q=NQ):
    td = _td(dt)
    M, d = n_q * n_win, 64 * H
    q, xk, xv = _dev(c.q.reshape(M, d), td), _dev(c.K, td), _dev(c.V, td)
    out = torch.full((A.tiled_elems(M, d),), A.SENTINEL, device="cuda", dtype=td)
    E.State.dbg_cross_attn_chunk(dt, q.data_ptr(), xk.data_ptr(), xv.data_ptr(), out.data_ptr(), n_win, H, t_len, win_len=lens, done=done,
                                 stream=torch.cuda.current_stream().cuda_stream, n_q=n_q)
    torch.cuda.synchronize()
    idx = torch.from_numpy(A.act_tiled_index(M, d)).cuda()
    return out[idx].double().cpu().numpy()


def _check(name, pattern, dt, got, ref):
    err = A.worst_error(got, ref)
    print(f"needles chunk16 {name} {pattern} {'bf16' if dt == 0 else 'f16'}: worst error {err:.3e} = {err / A.TOL[dt]:.3f} tol")
    assert err <= A.TOL[dt]


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("pattern", A.PATTERNS)
@pytest.mark.parametrize("t_len", T_LENS)
def test_chunk16_needles_uniform(E, t_len, pattern, dt):
    c, ref = _case(pattern, W, t_len)
    _check(f"t{t_len}", pattern, dt, _run(E, c, dt, W, t_len), ref)


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("pattern", A.PATTERNS)
@pytest.mark.parametrize("t_len,lens", [(200, [1, 200]), (97, [33, 97])])
def test_chunk16_needles_window_lengths(E, t_len, lens, pattern, dt):
    """per-window lengths: the slab stride stays t_len, the keys past a window's length are poison"""
    c, ref = _case(pattern, W, t_len, lens)
    _check(f"var{lens[0]}", pattern, dt, _run(E, c, dt, W, t_len, lens=lens), ref)


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("lens", [None, [33, 97, 5]])
def test_chunk16_done_window_keeps_sentinel(E, lens, dt):
    done = np.array([0, 1, 0], dtype=np.int32)
    c, ref = _case("sharp", 3, 97, lens)
    got = _run(E, c, dt, 3, 97, lens=lens, done=done)
    live = done[c.window] == 0
    _check("done" + ("_var" if lens else ""), "sharp", dt, got[live], ref[live])
    assert (got[~live] == A.SENTINEL).all()


@pytest.mark.parametrize("dt", [0, 1])
def test_all_16_rows_have_their_own_needle(E, dt):
    """every row of a window is decided by a key of its own, so an output that leaves rows 8..15 zero, or writes row i to row
    i - 8, is told apart - shown on the reference itself before the kernel is judged"""
    for k in range(64):
        c, ref = _case("sharp", W, 200, tag=f"own{k}")
        if all(len(set(c.needle[w * NQ:(w + 1) * NQ, h])) == NQ for w in range(W) for h in range(H)):
            break
    else:
        pytest.fail("no case with 16 distinct needles per window and head")
    zeroed = ref.copy()
    folded = ref.copy()
    for w in range(W):
        zeroed[w * NQ + 8:(w + 1) * NQ] = 0.0
        folded[w * NQ:w * NQ + 8] = ref[w * NQ + 8:(w + 1) * NQ]
    for bad in (zeroed, folded):
        rows = np.abs(bad - ref).max(axis=1)
        assert A.worst_error(bad, ref) > 100 * A.TOL[dt] and (rows > 100 * A.TOL[dt]).sum() >= 8 * W
    _check("own", "sharp", dt, _run(E, c, dt, W, 200), ref)


def test_chunk_entry_refuses_other_row_counts(E):
    """the refusal comes before any device work: the pointers are never dereferenced"""
    buf = torch.zeros(64, device="cuda", dtype=torch.bfloat16)
    p = buf.data_ptr()
    for n_q in (0, 4, 12, 32, -8):
        with pytest.raises(E.WhisperError) as ei:
            E.State.dbg_cross_attn_chunk(0, p, p, p, p, 2, 2, 64, n_q=n_q)
        assert ei.value.code == E.OHW_E_INVALID_ARG and "8 or 16" in str(ei.value)
