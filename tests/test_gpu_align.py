"""Word-timestamp alignment on the GPU (align.hip; ohw_state_set_align_heads / ohw_state_align and the ohw_dbg_align_* /
ohw_dbg_dtw entries).  Micro dimensions throughout; the one workload-sized case is the (225, 1500) DTW.

What is exact: the DTW (bit-defined), the start indices, the zeros past n_keys.  What is toleranced: the tap's soft-max
(TAP_TOL, measured as the header of check 3 says) and the reduction (align_ref.reduce_bound, derived)."""
import numpy as np
import pytest

from openhush_amd import synth

import align_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MICRO = synth.PRESETS["micro"]
ENV = 192
LENS = [64, 128, 192]
FRAMES = [3000, 200, 3000]          # window 1: n_frames / 2 = 100 keys, below its context of 128
N_KEYS = [64, 100, 192]
HEADS = [(0, 1), (1, 3)]            # two heads in two different layers
# Tap tolerance: worst |p_device - p_float64| over a row, relative to the row's largest probability, where p_float64 is
# computed from the same 16-bit inputs.  Measured on an MI355X over every case of test_tap_needles (both dtypes):
# worst observed 9.17e-7 (60 cases; the end-to-end cases below reached 5.83e-7); the tolerance is 4 x that (the factor covers
# summation-order changes across kernel variants).
TAP_OBSERVED = 9.17e-7
TAP_TOL = 4 * TAP_OBSERVED


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from openhush_amd import engine
    assert hasattr(engine.lib(), "ohw_state_align")
    return engine


@pytest.fixture(scope="module")
def ctxs(E):
    return {dt: E.Context.synthetic(MICRO.as_list(), 1234, 0, dt) for dt in (0, 1)}


def _td(dt):
    return torch.bfloat16 if dt == 0 else torch.float16


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the DTW kernel equals its host twin exactly
# ---------------------------------------------------------------------------------------------------------------------------
DTW_SHAPES = [(n, k) for n in (1, 2, 9, 40) for k in (1, 2, 7, 65)] + [(8, 64), (9, 65), (40, 200), (225, 1500)]


@pytest.mark.parametrize("n,k", DTW_SHAPES)
def test_dtw_kernel_equals_the_host_twin(E, n, k):
    rng = np.random.default_rng(7 * n + k)
    m = rng.standard_normal((n, k)).astype(np.float32)
    want = E.dtw(m)
    got = E.dtw(m, device=0)
    assert R.starts_wrong(want, got) == 0, (n, k, want.tolist()[:16], got.tolist()[:16])


def test_dtw_kernel_on_planted_and_tied_matrices(E):
    for n in (1, 9, 40):
        m, want = R.planted_diagonal(n)
        assert R.starts_wrong(want, E.dtw(m, device=0)) == 0, n
    for n, k in ((9, 9), (9, 2), (40, 65), (300, 40)):         # 300 rows: more rows than the workgroup has threads
        m = np.full((n, k), 0.5, dtype=np.float32)
        assert R.starts_wrong(E.dtw(m), E.dtw(m, device=0)) == 0, (n, k)
    rng = np.random.default_rng(1)
    m = rng.standard_normal((300, 40)).astype(np.float32)
    assert R.starts_wrong(E.dtw(m), E.dtw(m, device=0)) == 0


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the reduction kernels against the host twin and float64
# ---------------------------------------------------------------------------------------------------------------------------
def _probs(rng, A, n_all, n_keys, scale):
    lg = rng.standard_normal((A, n_all, n_keys)) * scale
    e = np.exp(lg - lg.max(axis=2, keepdims=True))
    return (e / e.sum(axis=2, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("n_keys", [1, 3, 7, 64, 300])
@pytest.mark.parametrize("A,n_all,n_prompt", [(1, 5, 4), (1, 30, 4), (2, 12, 4), (5, 30, 2)])
def test_reduce_kernels_against_the_host_twin(E, n_keys, A, n_all, n_prompt):
    rng = np.random.default_rng(n_keys * 1000 + A * 10 + n_all)
    p = _probs(rng, A, n_all, n_keys, 4.0 if A == 2 else 1.0)
    if n_keys >= 3:
        p[:, :, 1] = 0.25           # std == 0 columns
        p[0, :, 2] = 0.0
    host = E.align_reduce(p, n_prompt)
    dev = E.align_reduce(p, n_prompt, device=0)
    bound = R.reduce_bound(p, n_prompt)
    want = R.reduce_ref(p, n_prompt)
    e_host = float(np.abs(dev.astype(np.float64) - host).max())
    e_ref = np.abs(dev.astype(np.float64) - want)
    n_bits = int((dev.view(np.int32) != host.view(np.int32)).sum())
    print(f"reduce n_keys {n_keys} A {A} n_all {n_all}: device vs host max {e_host:.3g} ({n_bits} of {dev.size} values differ in bits), "
          f"device vs float64 max {float(e_ref.max()):.3g}, bound {bound.min():.3g} .. {bound.max():.3g}")
    assert np.isfinite(bound).all()
    assert (e_ref <= bound).all()
    assert (np.abs(dev.astype(np.float64) - host) <= bound).all()
    # the z-scores are the same fp32 operations on both sides, so an identical median selection gives identical bits (with one
    # head m IS the selected z value; with more, the head mean is the same sequential sum)
    assert n_bits == 0, n_bits


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the tap kernel, needle style
# ---------------------------------------------------------------------------------------------------------------------------
def _tap_case(dt, t_len, n_keys, rows, seed):
    H = 4
    rng = np.random.default_rng(seed)
    td = _td(dt)
    q = torch.from_numpy(rng.standard_normal((rows, H * 64)).astype(np.float32)).to(device="cuda", dtype=td)
    k = rng.standard_normal((H, t_len, 64)).astype(np.float32)
    qf = q.float().cpu().numpy()
    for h in range(H):
        for i in range(rows):                       # the needle of row i: one key that lines up with its query
            k[h, (i * 37 + h * 11) % n_keys] = qf[i, h * 64:(h + 1) * 64] * 0.5
        k[h, n_keys:] = 6e4 * np.where(rng.random((t_len - n_keys, 64)) < 0.5, -1.0, 1.0)       # poison: never to be read
    xk = torch.from_numpy(k).to(device="cuda", dtype=td)
    return q, xk, H


TAP_CASES = [(t, nk, r) for t in (7, 63, 64, 65, 200) for nk in sorted({1, t - 1, t}) for r in (1, 8)]


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("t_len,n_keys,rows", TAP_CASES)
def test_tap_needles(E, dt, t_len, n_keys, rows):
    q, xk, H = _tap_case(dt, t_len, n_keys, rows, 1000 * t_len + 10 * n_keys + rows)
    heads = [3, 0, 2]
    p = E.dbg_align_probs(dt, q.data_ptr(), xk.data_ptr(), rows, H, t_len, n_keys, heads, torch.cuda.current_stream().cuda_stream)
    qs = q.float().cpu().numpy().astype(np.float64) * 0.125
    kf = xk.float().cpu().numpy().astype(np.float64)
    worst = 0.0
    for a, h in enumerate(heads):
        want = R.softmax_ref(qs[:, h * 64:(h + 1) * 64], kf[h], n_keys)
        assert not p[a, :, n_keys:].any(), "a key at or past n_keys has a probability"
        assert np.isfinite(p[a]).all()
        rel = np.abs(p[a].astype(np.float64) - want).max(axis=1) / want.max(axis=1)
        worst = max(worst, float(rel.max()))
        assert np.abs(p[a].astype(np.float64).sum(axis=1) - 1.0).max() < 1e-5
    print(f"tap dt {dt} t_len {t_len} n_keys {n_keys} rows {rows}: worst relative error {worst:.3g} (tolerance {TAP_TOL:.3g})")
    assert worst <= TAP_TOL, worst


# ---------------------------------------------------------------------------------------------------------------------------
# 4 / 5. end to end on a state
# ---------------------------------------------------------------------------------------------------------------------------
PCM = np.stack([synth.synth_audio(7), synth.synth_audio(11), synth.synth_audio(13)])


def _state(E, ctx, windows=(0, 1, 2), lens=None, env=ENV, invariant=False):
    st = E.State(ctx, len(windows))
    st.set_batch_invariant(invariant)
    st.set_audio_ctx(env)
    if lens is not None:
        st.set_window_ctx(lens)
    st.mel(PCM[list(windows)], [synth.CHUNK_SAMPLES] * len(windows), E.OHW_MEL_ZERO_TAIL, want=False)
    st.encode(len(windows))
    return st


def _params(ctx, force_len):
    p = ctx.default_params()
    p.no_timestamps = 1             # every decoded token is a text token
    p.force_len = force_len
    return p


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("force_len", [1, 8, 9, 20])
def test_align_end_to_end(E, ctxs, dt, force_len):
    ctx = ctxs[dt]
    st = _state(E, ctx, lens=LENS)
    p = _params(ctx, force_len)
    toks, _ = st.greedy(3, p)
    assert all(len(t) == force_len and max(t) < ctx.tok.eot for t in toks)
    st.set_align_heads(HEADS)
    captures = st.counter("step_captures")
    idx = st.align(toks, FRAMES, p)
    assert st.counter("step_captures") == captures
    d = MICRO.n_text_state
    xk = {l: st.fetch(f"xk{l}", 3) for l, _ in HEADS}
    P = 4
    for b in range(3):
        nk, n_all, N = N_KEYS[b], P + force_len + 1, force_len + 1
        qv = st.fetch("align_q", b + 1)
        pv = st.fetch("align_p", b + 1)
        mv = st.fetch("align_m", b + 1)
        assert qv.shape == (n_all, 2, 64) and pv.shape == (2, n_all, nk) and mv.shape == (N, nk)
        # (a) the probabilities against float64 from the tapped queries and the layer's K
        p64 = np.zeros((2, n_all, nk))
        for a, (l, h) in enumerate(HEADS):
            p64[a] = R.softmax_ref(qv[:, a], xk[l][b, :, h * 64:(h + 1) * 64], nk)[:, :nk]
        rel = float((np.abs(pv - p64).max(axis=2) / p64.max(axis=2)).max())
        assert np.abs(pv.astype(np.float64).sum(axis=2) - 1.0).max() < 1e-5
        # (b) m against the float64 reduction of the fetched probabilities
        bound = R.reduce_bound(pv, P)
        e_m = np.abs(mv - R.reduce_ref(pv, P))
        # (c) the indices are the host DTW of the fetched m, exactly
        assert R.starts_wrong(E.dtw(mv), idx[b]) == 0, (b, E.dtw(mv).tolist(), idx[b].tolist())
        # (d) the returned path costs, on the all-float64 matrix, no more than the float64 optimum plus (path length) x bound.
        # bound: the path is optimal for the device's m, and both it and the float64 optimum are priced on a matrix that
        # differs from the device's by at most `cell` per cell (the reduction bound with the tap tolerance as input error) -
        # hence 2 x cell - plus the fp32 rounding of one running sum of at most L terms
        start, path = R.dtw_ref(mv)
        assert R.starts_wrong(start, idx[b]) == 0
        m64 = R.reduce_ref(p64, P)
        cell = float(R.reduce_bound(p64, P, p_err=TAP_TOL * float(p64.max())).max())
        L = len(path)
        bound_d = 2 * cell + R.U * L * float(np.abs(m64).max())
        excess = R.path_cost64(m64, path) - R.optimum64(m64)
        print(f"e2e dt {dt} force_len {force_len} window {b}: tap rel err {rel:.3g} (tol {TAP_TOL:.3g}); m err {float(e_m.max()):.3g} "
              f"(bound {bound.min():.3g} .. {bound.max():.3g}); path of {L} cells, excess cost {excess:.3g} (allowed {L * bound_d:.3g})")
        assert rel <= TAP_TOL
        assert np.isfinite(bound).all() and (e_m <= bound).all()
        assert np.isfinite(bound_d) and -1e-9 <= excess <= L * bound_d
        # invariants
        assert len(idx[b]) == N and np.all(np.diff(idx[b]) >= 0) and idx[b][0] >= 0 and idx[b][-1] <= nk - 1
    # a greedy decode after the alignment gives the tokens it gave before (the stale self K/V is rewritten from position 0)
    again, _ = st.greedy(3, p)
    assert again == toks
    st.close()


@pytest.mark.parametrize("dt", [0, 1])
def test_alignment_is_batch_invariant_and_skips_empty_windows(E, ctxs, dt):
    ctx = ctxs[dt]
    p = _params(ctx, 9)
    st = _state(E, ctx, lens=LENS, invariant=True)
    toks, _ = st.greedy(3, p)
    st.set_align_heads(HEADS)
    idx = st.align(toks, FRAMES, p)
    # window 1 skipped: its row is left alone, the others do not change
    part = st.align([toks[0], [], toks[2]], FRAMES, p)
    assert len(part[1]) == 0 and np.array_equal(part[0], idx[0]) and np.array_equal(part[2], idx[2])
    with pytest.raises(E.WhisperError):
        st.fetch("align_m", 2)
    st.close()
    for b in range(3):                              # each window alone, at its own context
        one = _state(E, ctx, windows=(b,), env=LENS[b], invariant=True)
        one.set_align_heads(HEADS)
        alone = one.align([toks[b]], [FRAMES[b]], p)
        assert np.array_equal(alone[0], idx[b]), (b, alone[0].tolist(), idx[b].tolist())
        one.close()


def test_align_under_a_language_table_uses_each_windows_language(E, ctxs):
    ctx = ctxs[1]
    p = _params(ctx, 8)
    st = _state(E, ctx, lens=LENS, invariant=True)
    st.set_align_heads(HEADS)
    st.set_window_lang([3, 17, 0])
    toks, _ = st.greedy(3, p)
    idx = st.align(toks, FRAMES, p)
    q_tab = st.fetch("align_q", 2)
    st.set_window_lang(None)
    p.lang_id = 17
    same = st.align(toks, FRAMES, p)
    assert np.array_equal(st.fetch("align_q", 2), q_tab) and np.array_equal(same[1], idx[1])
    p.lang_id = 5
    st.align(toks, FRAMES, p)
    assert not np.array_equal(st.fetch("align_q", 2), q_tab)      # the language token is part of the replayed sequence
    st.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. refusals: OHW_E_INVALID_ARG, the message names what is wrong
# ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(E, ctxs):
    ctx = ctxs[0]
    st = _state(E, ctx, lens=LENS)
    p = _params(ctx, 4)
    toks, _ = st.greedy(3, p)
    half = MICRO.n_text_ctx // 2

    def refused(f, *words):
        with pytest.raises(E.WhisperError) as e:
            f()
        assert e.value.code == E.OHW_E_INVALID_ARG, (e.value.code, str(e.value))
        for w in words:
            assert w in str(e.value), (w, str(e.value))

    refused(lambda: st.align(toks, FRAMES, p), "no alignment heads")
    refused(lambda: st.set_align_heads([(0, 1), (2, 0)]), "entry 1", "layer 2")
    refused(lambda: st.set_align_heads([(0, 0), (1, 1), (1, 4)]), "entry 2", "head 4")
    refused(lambda: st.set_align_heads([(0, -1)]), "entry 0")
    refused(lambda: st.set_align_heads([(0, 0)] * 33), "33 heads")
    refused(lambda: st.align(toks, FRAMES, p), "no alignment heads")           # a refused list sets nothing
    st.set_align_heads([(0, 0)] * 32)                                          # the limit itself is fine
    st.set_align_heads(HEADS)
    bad = [list(t) for t in toks]
    bad[2][1] = ctx.tok.eot
    refused(lambda: st.align(bad, FRAMES, p), "window 2", "token 1")
    bad[2][1] = ctx.tok.timestamp_begin + 3
    refused(lambda: st.align(bad, FRAMES, p), "window 2", "token 1")
    bad[2][1] = -1
    refused(lambda: st.align(bad, FRAMES, p), "window 2", "token 1")
    refused(lambda: st.align([toks[0], [7] * (half + 1), toks[2]], FRAMES, p), "window 1", str(half + 1))
    st.align([toks[0], [7] * half, toks[2]], FRAMES, p)                        # n_text_ctx / 2 tokens fit
    refused(lambda: st.align(toks[:2], FRAMES[:2], p), "batch")
    st.set_window_lang([0, E.OHW_LANG_DETECT, 0])
    refused(lambda: st.align(toks, FRAMES, p), "window 1", "language")
    st.set_window_lang(None)
    st.set_audio_ctx(128)                                                      # clears the lengths, changes the context
    refused(lambda: st.align(toks, FRAMES, p), "audio context")
    st.set_audio_ctx(ENV)
    refused(lambda: st.align(toks, FRAMES, p), "per-window contexts")
    st.set_window_ctx(LENS)
    assert len(st.align(toks, FRAMES, p)) == 3
    st.set_align_heads(None)
    refused(lambda: st.align(toks, FRAMES, p), "no alignment heads")
    st.close()


# ---------------------------------------------------------------------------------------------------------------------------
# the replay is the teacher-forced sequence; packed encoder; validity of the fetches
# ---------------------------------------------------------------------------------------------------------------------------
def test_replay_rows_do_not_depend_on_what_follows_them(E, ctxs):
    # teacher forcing is causal: the tapped query rows of the prompt and the first 9 tokens are the same bits whether 9 or 20
    # tokens are replayed (a wrong chunk layout, position or prompt moves them), and they differ once a token differs
    ctx = ctxs[1]
    st = _state(E, ctx, lens=LENS, invariant=True)
    toks, _ = st.greedy(3, _params(ctx, 20))
    st.set_align_heads(HEADS)
    p = _params(ctx, 20)
    st.align(toks, FRAMES, p)
    q20 = [st.fetch("align_q", b + 1) for b in range(3)]
    st.align([t[:9] for t in toks], FRAMES, p)
    for b in range(3):
        q9 = st.fetch("align_q", b + 1)
        assert q9.shape[0] == 4 + 9 + 1 and np.array_equal(q9[:13], q20[b][:13]), b
    other = [list(t[:9]) for t in toks]
    other[1][4] = (other[1][4] + 1) % 1000
    st.align(other, FRAMES, p)
    q = st.fetch("align_q", 2)
    assert np.array_equal(q[:8], q20[1][:8]) and not np.array_equal(q[8], q20[1][8])      # row P + 4 is the changed token
    assert np.array_equal(st.fetch("align_q", 1)[:13], q20[0][:13])                      # the other windows do not move
    # an encode ends the validity of the fetches
    st.mel(PCM, [synth.CHUNK_SAMPLES] * 3, E.OHW_MEL_ZERO_TAIL, want=False)
    st.encode(3)
    with pytest.raises(E.WhisperError):
        st.fetch("align_m", 1)
    st.close()
    fresh = E.State(ctx, 1)
    with pytest.raises(E.WhisperError):
        fresh.fetch("align_q", 1)
    fresh.close()


def test_alignment_under_the_packed_encoder(E, ctxs):
    ctx = ctxs[0]
    p = _params(ctx, 9)
    res = []
    for packed in (False, True):
        st = E.State(ctx, 3)
        st.set_batch_invariant(True)
        st.set_audio_ctx(ENV)
        st.set_window_ctx(LENS)
        st.set_packed_encoder(packed)
        st.mel(PCM, [synth.CHUNK_SAMPLES] * 3, E.OHW_MEL_ZERO_TAIL, want=False)
        st.encode(3)
        assert st.counter("enc_rows") == (sum(LENS) if packed else 3 * ENV)
        toks, _ = st.greedy(3, p)
        st.set_align_heads(HEADS)
        res.append((toks, st.align(toks, FRAMES, p)))
        st.close()
    assert res[0][0] == res[1][0]
    for b in range(3):
        assert np.array_equal(res[0][1][b], res[1][1][b]), b


# ---------------------------------------------------------------------------------------------------------------------------
# 7. the engine
# ---------------------------------------------------------------------------------------------------------------------------
def _recording():
    a = np.concatenate([synth.synth_audio(21), synth.synth_audio(22), synth.synth_audio(23)])
    return a[:70 * 16000].copy()


def _run_engine(E, path, heads, schedule):
    eng = E.WhisperEngine.new(path, "en", False, True, 0, E.OHW_DTYPE_F16, 1)
    eng.set_decode_policy(temperature_inc=0.0)
    E.lib().ohw_engine_set_force_len(eng.h, 12)
    eng.set_schedule(schedule, lanes=2, merge=1)
    eng.set_word_timestamps(heads)
    r = eng.transcribe(E.AudioBuffer(_recording(), 16000))
    out = dict(text=r.text, tokens=eng.last_tokens(), times=eng.last_token_times(), words=eng.last_words(), segments=eng.last_segments(),
               quality=eng.last_quality_ex(), raw=eng._last_text_bytes())
    eng.close()
    return out


def test_engine_word_timestamps(E, ctxs, tmp_models):
    path = tmp_models("micro")
    ctx = ctxs[1]
    off = _run_engine(E, path, None, E.OHW_SCHEDULE_SEQUENTIAL)
    seq = _run_engine(E, path, HEADS, E.OHW_SCHEDULE_SEQUENTIAL)
    lanes = _run_engine(E, path, HEADS, E.OHW_SCHEDULE_LANES)
    # the setting changes neither tokens nor text; off: no token times, no words, segments all the same
    assert off["tokens"] == seq["tokens"] == lanes["tokens"] and off["text"] == seq["text"] == lanes["text"]
    assert off["times"] == [] and off["words"] == [] and off["segments"] == seq["segments"] and len(off["segments"]) > 0
    assert seq["times"] == lanes["times"] and seq["words"] == lanes["words"] and seq["segments"] == lanes["segments"]
    assert len(seq["quality"]) == 3
    eot = ctx.tok.eot
    assert [t["id"] for t in seq["times"]] == [t for t in seq["tokens"] if t < eot]
    raw, dur = seq["raw"], 70.0
    for w in range(3):
        tt = [t for t in seq["times"] if t["window"] == w]
        assert len(tt) > 0
        lo, hi = 30.0 * w, min(30.0 * w + 30.0, dur)
        assert all(a["t0"] <= a["t1"] for a in tt) and all(a["t1"] <= b["t0"] + 1e-6 for a, b in zip(tt, tt[1:]))
        assert tt[0]["t0"] >= lo - 1e-4 and tt[-1]["t1"] <= hi + 1e-4, (w, tt[0], tt[-1])
    # words: the host rule on every window's token bytes, each word slicing the text to its tokens' bytes
    _check_words(E, ctx, seq)
    for s in seq["segments"]:
        assert 0.0 <= s["t0"] <= s["t1"] <= dur + 1e-4 and s["text_len"] > 0
    # the engine was created with language "en"; turning the setting off gives the buffers back and the times stop
    eng = E.WhisperEngine.new(path, "en", False, True, 0, E.OHW_DTYPE_F16, 1)
    with pytest.raises(E.WhisperError) as ex:
        eng.set_word_timestamps([(0, 0), (5, 0)])
    assert ex.value.code == E.OHW_E_INVALID_ARG and "entry 1" in str(ex.value)
    eng.close()


def _check_words(E, ctx, seq):
    """every word slices the text to exactly its tokens' bytes; only the recording's first / last word can lose white space to
    the trim of the text's two ends"""
    raw = seq["raw"]
    n_words = len(seq["words"])
    words = list(seq["words"])
    joined = b""
    for w in range(3):
        tt = [t for t in seq["times"] if t["window"] == w]
        tb = [ctx.token_text(t["id"]) for t in tt]
        starts = E.word_starts(tb)
        groups = []
        for k, s in enumerate(starts):
            if s:
                groups.append([])
            groups[-1].append(k)
        for g in groups:
            wd = words.pop(0)
            want = b"".join(tb[k] for k in g)
            got = raw[wd["text_off"]:wd["text_off"] + wd["text_len"]]
            joined += want
            idx = n_words - len(words) - 1
            if idx == 0:
                want = want.lstrip(b" \t\r\n")
            if idx == n_words - 1:
                want = want.rstrip(b" \t\r\n")
            assert got == want and (len(got) > 0 or idx in (0, n_words - 1)), (idx, got, want)
            assert wd["t0"] == tt[g[0]]["t0"] and wd["t1"] == tt[g[-1]]["t1"]
    assert words == [] and joined.strip(b" \t\r\n") == raw


def test_pool_gathers_the_engines_times(E, ctxs, tmp_models):
    # two engines on one device take windows 0, 2 and 1 of the 70 s recording: tokens, text and all three arrays must be the
    # single engine's, re-indexed into the pool's text and the recording's windows
    path = tmp_models("micro")
    ctx = ctxs[1]
    one = _run_engine(E, path, HEADS, E.OHW_SCHEDULE_SEQUENTIAL)
    pool = E.EnginePool(path, "en", False, [0, 0], E.OHW_DTYPE_F16, 1)
    pool.set_decode_policy(temperature_inc=0.0)
    pool.set_force_len(12)
    r = pool.transcribe(E.AudioBuffer(_recording(), 16000))
    assert pool.last_token_times() == [] and pool.last_words() == [] and pool.last_segments() == one["segments"]
    pool.set_word_timestamps(HEADS)
    r = pool.transcribe(E.AudioBuffer(_recording(), 16000))
    got = dict(text=r.text, tokens=pool.last_tokens(), times=pool.last_token_times(), words=pool.last_words(),
               segments=pool.last_segments(), raw=pool._last_text_bytes())
    assert got["text"] == one["text"] and got["tokens"] == one["tokens"]
    assert got["times"] == one["times"] and got["words"] == one["words"] and got["segments"] == one["segments"]
    assert sorted({t["window"] for t in got["times"]}) == [0, 1, 2]
    _check_words(E, ctx, got)
    with pytest.raises(E.WhisperError):
        pool.set_word_timestamps([(9, 0)])
    pool.set_word_timestamps(None)
    pool.transcribe(E.AudioBuffer(_recording(), 16000))
    assert pool.last_token_times() == [] and pool.last_segments() == one["segments"]
    pool.close()


def test_a_refused_align_ends_the_validity_of_the_fetches(E, ctxs):
    ctx = ctxs[0]
    st = _state(E, ctx, lens=LENS)
    p = _params(ctx, 4)
    toks, _ = st.greedy(3, p)
    st.set_align_heads(HEADS)
    st.align(toks, FRAMES, p)
    assert st.fetch("align_m", 1).shape == (5, N_KEYS[0])
    bad = [list(t) for t in toks]
    bad[0][0] = ctx.tok.eot
    with pytest.raises(E.WhisperError):
        st.align(bad, FRAMES, p)
    assert st.fetch("align_m", 1).shape == (5, N_KEYS[0])          # refused before anything changed: the last alignment stands
    st.set_align_heads(None)
    with pytest.raises(E.WhisperError):
        st.fetch("align_m", 1)
    st.close()
