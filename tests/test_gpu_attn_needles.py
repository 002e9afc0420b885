"""The attention kernels against a float64 reference on needle inputs (tests/attn_needles.py): one key, or an exactly known
pair, decides every output, and every key a query must not see is poison, so a dropped, extra or misplaced key shows as an
error of tens of tolerances.  Encoder attention (uniform, per-window lengths, packed rows), cross-attention (every variant
launch_cross_attn picks, asserted) and masked self-attention (plain and with the beam slot table) run through the dbg entries
on caller data; outputs are pre-filled with a sentinel that rows a contract leaves unstored must keep.

Tolerance (attn_needles.TOL): 2^-7 (bf16) / 2^-10 (f16) times max|V| = 1, from the number formats alone.  Every case prints
its worst error.
"""
import ctypes as C

import numpy as np
import pytest

import attn_needles as A

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

WORST = {}     # (family, dtype) -> largest error seen, printed by every case


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
    return torch.from_numpy(np.array(a)).to(device="cuda", dtype=td)      # a copy: the cases are read-only


def _i32(x):
    return None if x is None else np.ascontiguousarray(x, dtype=np.int32)


def _ip(E, a):
    return None if a is None else E._ip(a)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _report(family, name, pattern, dt, err):
    key = (family, "bf16" if dt == 0 else "f16")
    WORST[key] = max(WORST.get(key, 0.0), err)
    print(f"needles {family} {name} {pattern} {key[1]}: worst error {err:.3e} = {err / A.TOL[dt]:.3f} tol; family so far {WORST[key]:.3e}")


def _untile(out, M, d):
    """rows [M][d] of an activation-tile buffer, and the elements of the buffer that belong to no row < M"""
    idx = torch.from_numpy(A.act_tiled_index(M, d)).cuda()
    rest = torch.ones(out.numel(), dtype=torch.bool, device="cuda")
    rest[idx.reshape(-1)] = False
    return out[idx].double().cpu().numpy(), out[rest]


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("pattern", A.PATTERNS)
@pytest.mark.parametrize("name", list(A.ENCODER_CASES))
def test_encoder_attention_needles(E, name, pattern, dt):
    B, T, H, lens, mode = A.ENCODER_CASES[name]
    c, ref, _ = A.make("encoder", name, pattern)
    d = 64 * H
    img, where = A.encoder_qkv(c, packed=mode == "packed", guard=3)
    qkv = _dev(img, _td(dt))
    out = torch.full((img.shape[0], d), A.SENTINEL, device="cuda", dtype=_td(dt))
    if mode == "uniform":
        rc = E.lib().ohw_dbg_attention(dt, qkv.data_ptr(), out.data_ptr(), B, T, H, _stream())
    else:
        wl = _i32(lens)
        wo = _i32(np.concatenate([[0], np.cumsum(lens)[:-1]])) if mode == "packed" else None
        rc = E.lib().ohw_dbg_attention_var(dt, qkv.data_ptr(), out.data_ptr(), B, T, H, _ip(E, wl), _ip(E, wo), _stream())
    assert rc == 0, E.last_error()
    torch.cuda.synchronize()
    got = out.double().cpu().numpy()
    err = A.worst_error(got[where], ref)
    _report("encoder", name, pattern, dt, err)
    assert err <= A.TOL[dt]
    if mode == "uniform":
        assert len(where) == B * T                      # every row is a query row
    elif mode == "var":
        for b, n in enumerate(lens):                    # query blocks (128 rows) wholly past the length: zeros
            first = -(-n // 128) * 128
            assert not got[b * T + first:(b + 1) * T].any(), b
    else:
        assert len(where) == sum(lens)                  # every row belongs to one window and equals ITS reference ...
        assert (got[sum(lens):] == A.SENTINEL).all()    # ... and the three guard rows behind the last window are untouched


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("pattern", A.PATTERNS)
@pytest.mark.parametrize("name", list(A.CROSS_CASES))
def test_cross_attention_needles(E, name, pattern, dt):
    p = A.CROSS_CASES[name]
    c, ref, _ = A.make("cross", name, pattern)
    M, H, d = p["M"], 2, 128
    td = _td(dt)
    q, xk, xv = _dev(c.q.reshape(M, d), td), _dev(c.K, td), _dev(c.V, td)
    # the slices publish their states before the merge reads them: scratch starts as NaN, the tickets as zero
    partials = torch.full((M * H * A.XA_MAX_SPLIT * 68,), float("nan"), device="cuda") if p["scratch"] else None
    tickets = torch.zeros(M * H, device="cuda", dtype=torch.int32) if p["scratch"] else None
    done, lens = _i32(p["done"]), _i32(p["lens"])
    want_variant = getattr(E, "XA_" + p["variant"].upper())
    split = p["variant"] in ("split", "group_split")
    outs = []
    for _ in range(2 if split else 1):
        out = torch.full((A.tiled_elems(M, d),), A.SENTINEL, device="cuda", dtype=td)
        variant = C.c_int(-1)
        rc = E.lib().ohw_dbg_cross_attn(dt, q.data_ptr(), xk.data_ptr(), xv.data_ptr(), out.data_ptr(), M, p["n_new"], H, p["t_len"],
                                        p["kv_group"], int(p["invariant"]), _ip(E, done), _ip(E, lens),
                                        partials.data_ptr() if p["scratch"] else None, tickets.data_ptr() if p["scratch"] else None,
                                        M, C.byref(variant), _stream())
        assert rc == 0, E.last_error()
        torch.cuda.synchronize()
        assert variant.value == want_variant, (name, variant.value, want_variant)
        if p["scratch"]:
            assert not tickets.any()                    # the last arriver re-arms its ticket
        outs.append(out)
    if split:
        assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))       # same buffers, same bits
        assert A.xa_slices(p) == {63: 1, 250: 2, 1500: 8}[p["t_len"]]
    got, rest = _untile(outs[0], M, d)
    live = np.ones(M, dtype=bool) if done is None else done[c.window] == 0
    err = A.worst_error(got[live], ref[live])
    _report("cross", f"{name} [{p['variant']}]", pattern, dt, err)
    assert err <= A.TOL[dt]
    assert (got[~live] == A.SENTINEL).all()             # the rows of finished windows are not stored
    assert (rest == A.SENTINEL).all()                   # nor anything past row M - 1 of the last tile


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("pattern", A.PATTERNS)
@pytest.mark.parametrize("name", list(A.SELF_CASES))
def test_self_attention_needles(E, name, pattern, dt):
    n_new, slots = A.SELF_CASES[name]
    c, ref, _ = A.make("self", name, pattern)
    M, H, d = len(A.N_PAST) * n_new, 2, 128
    td = _td(dt)
    q, kc, vc = _dev(c.q.reshape(M, d), td), _dev(c.K, td), _dev(c.V, td)
    out = torch.full((A.tiled_elems(M, d),), A.SENTINEL, device="cuda", dtype=td)
    variant = C.c_int(-1)
    rc = E.lib().ohw_dbg_self_attn(dt, q.data_ptr(), kc.data_ptr(), vc.data_ptr(), _ip(E, _i32(A.N_PAST)), out.data_ptr(), M, n_new, H,
                                   A.N_CTX, _ip(E, _i32(c.table)), C.byref(variant), _stream())
    assert rc == 0, E.last_error()
    torch.cuda.synchronize()
    assert variant.value == (E.SA_SLOTS if slots else E.SA_PLAIN)
    got, rest = _untile(out, M, d)
    err = A.worst_error(got, ref)
    _report("self", name, pattern, dt, err)
    assert err <= A.TOL[dt]
    assert (rest == A.SENTINEL).all()


def test_dbg_entries_refuse_bad_tables(E):
    """every refusal comes before any device work: the pointers are never dereferenced (nothing is launched)"""
    L = E.lib()
    buf = torch.zeros(64, device="cuda", dtype=torch.bfloat16)
    ptr = buf.data_ptr()

    def refused(rc, word):
        assert rc == E.OHW_E_INVALID_ARG, rc
        assert word in E.last_error(), E.last_error()

    def att(lens, offs):
        return L.ohw_dbg_attention_var(0, ptr, ptr, 2, 300, 2, _ip(E, _i32(lens)), _ip(E, _i32(offs)), None)
    refused(att([300, 0], None), "win_len[1] = 0")                       # a length 0
    refused(att([301, 5], None), "win_len[0] = 301")                     # a length > T
    refused(att([300, 5], [0, 299]), "prefix sum")                       # offsets that are not the prefix sum
    refused(att(None, [0, 300]), "need the windows' lengths")

    def xa(M=4, n_new=1, t_len=250, kv_group=1, lens=None, scratch=False, max_rows=0):
        return L.ohw_dbg_cross_attn(0, ptr, ptr, ptr, ptr, M, n_new, 2, t_len, kv_group, 0, None, _ip(E, _i32(lens)),
                                    ptr if scratch else None, ptr if scratch else None, max_rows, None, None)
    refused(xa(M=6, kv_group=6), "kv_group")
    refused(xa(M=5, n_new=2), "multiple of n_new")
    refused(xa(M=5, kv_group=2), "multiple of kv_group")
    refused(xa(lens=[250, 0, 1, 1]), "win_len[1] = 0")
    refused(xa(lens=[250, 251, 1, 1]), "win_len[1] = 251")
    refused(xa(scratch=True, max_rows=3), "max_split_rows")

    def sa(n_past, n_new=1, n_ctx=448, table=None):
        return L.ohw_dbg_self_attn(0, ptr, ptr, ptr, _ip(E, _i32(n_past)), ptr, len(n_past) * n_new, n_new, 2, n_ctx, _ip(E, _i32(table)),
                                   None, None)
    refused(sa([0, 447], n_new=2), "n_past[1] = 447")                    # n_past + n_new > n_ctx
    refused(sa([0, -1]), "n_past[1] = -1")
    table = np.zeros((2, 448), dtype=np.int32)
    table[1, 5] = 2
    refused(sa([3, 9], table=table), "kv_slot[1][5] = 2")                # a slot out of range
    table[1, 5] = -1
    refused(sa([3, 9], table=table), "kv_slot[1][5] = -1")
