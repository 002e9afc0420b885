"""Every model width the loader accepts (128 .. 1280 in steps of 128), on the GPU.

Width picks template instantiations and launch shapes - layernorm_kernel's MAXV, dec_gemm_pick's work shape, the encoder
GEMM's kernel per N, the head count of every attention launch - and the rest of the suite builds models of width 128, 256,
384, 768 and 1280 only.  Here:

  (a) mel -> encoder -> decoder of a 2 + 2-layer model of every width, both dtypes, against the fp32 oracle
  (b) greedy and beam search of 5 at widths 512 and 1024 (8 and 16 heads), the oracle walking the GPU's own path
  (c) a 96-row lane at widths 512 and 1024 against the same windows in batches of 16, bit for bit, every GEMM's shape asserted
  (d) LayerNorm on both sides of every MAXV switch, the embedding at 512 / 1024, attention needles at 8 and 16 heads: float64
  (e) the first widths the loader refuses, and the last it accepts

Tolerances are those of test_gpu_parity.py (activations 6e-2 bf16 / 8e-3 f16, doubled behind a whole block; logits 0.25 /
0.03 absolute): test_widths_cpu.py shows the oracle's logit sigma is 4.0 at every width, which is what those absolute bounds
were set for.  A differing argmax is excused (f16) only under an oracle margin of twice the logit bound; test_widths_cpu.py
caps how many positions can be that thin.  In bf16 that threshold (0.5) covers half the positions, so picks are printed only.
"""
import ctypes as C
import os

import numpy as np
import pytest

import attn_needles as A
import dec_gemm_ref as R
import width_models as W
from openhush_amd import modelfile, synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DT_NAME = {0: "bf16", 1: "f16"}


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from openhush_amd import engine
    engine.lib()
    return engine


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o
    o.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    return o


@pytest.fixture(scope="module")
def pcm():
    p = W.windows()
    p.setflags(write=False)
    return p


def _tally(st):
    out = {}
    for n in W.tally_names():
        v = st.counter(n)
        if v:
            out[n] = v
    return out


def _short(tally):
    return " ".join(f"{k.replace('dec_gemm.', '')}={v}" for k, v in tally.items())


# ---------------------------------------------------------------------------------------------------------------------
# (a) the whole path
# ---------------------------------------------------------------------------------------------------------------------
_oracle_side = {}     # hparams -> (model, mel references, encoder references with taps): once per width, shared by both dtypes


def _reference(oracle, hp, pcm):
    key = tuple(hp)
    if key not in _oracle_side:
        om = oracle.Model.synth(hp, 1234)
        mels = [om.log_mel(pcm[b, :W.WINDOW_SAMPLES[b]], W.MEL_ZERO_TAIL) for b in range(2)]
        encs = [om.encode(m, taps=True) for m in mels]
        _oracle_side.clear()                      # one width's model at a time
        _oracle_side[key] = (om, mels, encs)
    return _oracle_side[key]


def _whole_path(E, oracle, pcm, hp, dt):
    """mel, encoder and 48 teacher-forced decoder positions of the two windows -> the figures the sweep prints"""
    d = hp[2]
    om, ref_mel, ref_enc = _reference(oracle, hp, pcm)
    ctx = E.Context.synthetic(hp, 1234, 0, dt)
    st = E.State(ctx, 2)
    mel = st.mel(np.array(pcm), list(W.WINDOW_SAMPLES), E.OHW_MEL_ZERO_TAIL)
    st.encode(2)
    enc = st.fetch("enc", 2)
    tol = W.TOL_ACT[dt]
    taps = d <= 512
    if taps:
        conv1, stem, block0 = (st.fetch(k, 2) for k in ("conv1", "stem", "block0"))
    worst_enc = 0.0
    for b in range(2):
        assert np.abs(mel[b] - ref_mel[b]).max() < 2e-4, (d, b)
        r_enc, r_c1, r_stem, r_b0 = ref_enc[b]
        assert np.isfinite(enc[b]).all()
        e = float(np.abs(enc[b] - r_enc).max())
        worst_enc = max(worst_enc, e)
        assert e < 2 * tol, (d, dt, b, e)
        if taps:
            assert np.abs(conv1[b] - r_c1).max() < tol, (d, dt, b)
            assert np.abs(stem[b] - r_stem).max() < tol, (d, dt, b)
            assert np.abs(block0[b] - r_b0).max() < 2 * tol, (d, dt, b)
    # the decoder alone: the oracle reads the GPU's encoder output
    forced = W.forced_tokens(d)
    ref = []
    for b in range(2):
        s = oracle.State(om)
        s.set_encoder_output(enc[b])
        ref.append(s.decode(forced, 0, all_pos=True))
        s.close()
    ltol = W.TOL_LOGIT[dt]
    worst = 0.0
    same = total = 0

    def row(got, b, pos):
        nonlocal worst, same, total
        want = ref[b][pos]
        err = float(np.abs(got - want).max())
        worst = max(worst, err)
        assert err < ltol, (d, DT_NAME[dt], b, pos, err)
        total += 1
        if int(got.argmax()) == int(want.argmax()):
            same += 1
        elif dt == 1:
            top = np.partition(want, -2)[-2:]
            assert top[1] - top[0] < 2 * ltol, (d, b, pos, int(got.argmax()), int(want.argmax()), float(top[1] - top[0]))

    f = np.asarray(forced, np.int32)
    lg = st.decode(np.tile(f[:4], (2, 1)), [0, 0])                       # the prompt pass
    for b in range(2):
        row(lg[b], b, 3)
    for i in range(4, 40):                                               # window 1 trails by one: its first step feeds position 3 again
        lg = st.decode(np.asarray([[f[i]], [f[i - 1]]], np.int32), [i, i - 1])
        row(lg[0], 0, i)
        row(lg[1], 1, i - 1)
    lg = st.decode(np.stack([f[40:48], f[39:47]]), [40, 39])             # eight tokens in one call, still ragged
    row(lg[0], 0, 47)
    row(lg[1], 1, 46)
    tally = _tally(st)
    st.close()
    ctx.close()
    print(f"width {d} {DT_NAME[dt]} layers {hp[4]}+{hp[8]}: encoder worst {worst_enc:.5f} (bound {2 * tol}), logits worst {worst:.5f} "
          f"(bound {ltol}), picks {same} / {total}; {_short(tally)}")
    return worst_enc, worst, same, total, tally


@pytest.mark.parametrize("dt", [1, 0], ids=["f16", "bf16"])
@pytest.mark.parametrize("d", W.WIDTHS)
def test_whole_path_matches_the_oracle_at_every_width(E, oracle, pcm, d, dt):
    _, _, same, total, tally = _whole_path(E, oracle, pcm, W.shallow(d), dt)
    assert total == 2 + 2 * 36 + 2
    # two layers, 38 calls: every GEMM counted in every call, on the fused LayerNorm forms, never on a lane shape
    for g in W.GEMMS:
        per_call = 1 if g == "logits" else 2
        n = sum(v for k, v in tally.items() if k.startswith(f"dec_gemm.{g}."))
        assert n == 38 * per_call, (g, tally)
    assert not any(k.endswith(s) for k in tally if k.startswith("dec_gemm.") for s in ("4x2", "1x6", "4x6", "5x6")), tally
    for M, calls in ((8, 1), (2, 36), (16, 1)):
        for g in W.GEMMS:
            assert tally.get(W.counter_name(g, W.dec_gemm_shape(g, M, d, 0)), 0) >= calls * (1 if g == "logits" else 2), (g, M, tally)


# ---------------------------------------------------------------------------------------------------------------------
# (b) greedy and beam search at 8 and 16 heads
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [512, 1024])
def test_greedy_and_beam_at_base_and_medium_width(E, oracle, pcm, d):
    dt = 1
    hp = W.shallow(d)
    om, ref_mel, ref_enc = _reference(oracle, hp, pcm)
    ctx = E.Context.synthetic(hp, 1234, 0, E.OHW_DTYPE_F16)
    bias = np.zeros(ctx.hp.n_vocab, np.float32)
    # test_gpu_persist.py's kind of bias, sized for these models (chosen on the oracle alone): a two-layer procedural model
    # repeats itself, so what varies is how a sequence ends - at 512 one window ends behind its first token and one after ten
    # steps, at 1024 text and timestamps alternate up to n_max and a beam finishes after eleven
    bias[ctx.tok.timestamp_begin:] = 4.0
    bias[ctx.tok.eot] = 17.0
    N_MAX, K = 16, 5
    st = E.State(ctx, 2 * K)
    st.set_logit_bias(bias)
    mel = st.mel(np.array(pcm), list(W.WINDOW_SAMPLES), E.OHW_MEL_ZERO_TAIL)
    st.encode(2)
    p = ctx.default_params(); p.n_max = N_MAX
    dev = st.greedy_ex(2, p)
    st.set_batch_invariant(True)         # two windows alone would take the key-split form: the variant rule of a full batch
    beams = st.beam_search(2, K, p)
    st.set_batch_invariant(False)
    tally = _tally(st)
    op = om.default_params(); op.n_max = N_MAX
    tol = W.TOL_LOGIT[dt]
    same = total = exact = 0
    for b in range(2):
        assert np.abs(mel[b] - ref_mel[b]).max() < 2e-4
        enc = ref_enc[b][0]
        # greedy: test_gpu_parity.py::test_greedy_tokens_match_oracle's rule
        s = oracle.State(om)
        s.set_encoder_output(enc)
        forced = dev[b]["tokens"] + ([om.tok_eot] if dev[b]["ended_by_eot"] else [])
        ref = s.greedy_ex(op, bias, forced)
        assert len(ref["choice"]) >= len(forced)
        lp_ok = True
        for i, t in enumerate(forced):
            total += 1
            if ref["choice"][i] == t:
                same += 1
                lp_ok = lp_ok and abs(float(dev[b]["logprobs"][i]) - float(ref["logprobs"][i])) < 2 * tol
            else:
                assert ref["margins"][i] < 2 * tol, (d, b, i, t, ref["choice"][i], float(ref["margins"][i]))
        assert lp_ok, (d, b)
        assert dev[b]["ended_by_eot"] or len(dev[b]["tokens"]) == N_MAX
        # beam search: test_gpu_beam.py's rule
        g = beams[b]
        rb = oracle.beam_search(om, enc, op, K, bias)
        assert len(g["tokens"]) > 0
        if g["tokens"] == rb["tokens"]:
            exact += 1
            assert abs(g["sum_logprob"] - rb["sum_logprob"]) < 0.06 * max(1, len(g["tokens"])) ** 0.5
        else:
            best = max(c[1] / max(1, len(c[0])) for c in rb["candidates"])
            mine = max(s.score_sequence(op, g["tokens"], e, bias) / max(1, len(g["tokens"])) for e in (True, False))
            assert mine > best - 0.02, (d, b, g, rb["tokens"], mine, best)
        ts = [t for t in g["tokens"] if t >= om.tok_beg]
        assert ts == sorted(ts)
        s.close()
    print(f"width {d} f16: greedy steps where the oracle picks the GPU's token {same} / {total}; beam winners equal {exact} / 2; {_short(tally)}")
    assert same >= 0.9 * total
    assert max(len(x["tokens"]) for x in dev) >= 8 and max(len(x["tokens"]) for x in beams) >= 8      # real steps, not two prompt passes
    assert tally.get("xattn.group5", 0) > 0 and tally.get("self_attn.slots", 0) > 0, tally
    st.close()
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# (c) a 96-row lane
# ---------------------------------------------------------------------------------------------------------------------
AUDIO_CTX = 64
N_LAYER = 2


def _lane_run(E, ctx, lane, lane_pcm, first, count):
    """test_gpu_lane_ln_forms.py's run: a two-token prompt pass and three single-token steps of `count` windows as ONE batch ->
    (the four logits arrays, the counters behind the prompt pass, the counters behind the steps)"""
    tok = ctx.tok
    prompt = np.asarray([tok.sot, tok.no_timestamps], np.int32)
    st = E.State(ctx, count)
    st.set_batch_invariant(True)
    st.set_stream(lane.ptr)
    st.set_audio_ctx(AUDIO_CTX)
    st.mel(lane_pcm[first:first + count], None, E.OHW_MEL_ZERO_TAIL, want=False)
    st.encode(count)
    logits = [st.decode(np.tile(prompt, (count, 1)), [0] * count)]
    in_prompt = _tally(st)
    for i in range(3):
        logits.append(st.decode(logits[-1].argmax(axis=1).astype(np.int32)[:, None], [2 + i] * count))
    after = _tally(st)
    in_steps = {k: v - in_prompt.get(k, 0) for k, v in after.items() if v - in_prompt.get(k, 0) > 0}
    st.close()
    return logits, in_prompt, in_steps


_lane_seen = set()


@pytest.mark.parametrize("d", W.LANE_WIDTHS)
def test_a_96_row_lane_gives_the_bits_of_16_row_batches(E, d):
    ctx = E.Context.synthetic(W.shallow(d), 4321, 0, E.OHW_DTYPE_BF16)
    lane = E.Stream(0, 0, W.LANE_CUS)
    lane_pcm = np.stack([synth.synth_audio(900 + w, AUDIO_CTX * 320) for w in range(W.LANE_ROWS)])
    ref = [[] for _ in range(4)]
    for f in range(0, W.LANE_ROWS, 16):
        logits, in_prompt, in_steps = _lane_run(E, ctx, lane, lane_pcm, f, 16)
        for t in (in_prompt, in_steps):
            assert not any(k.endswith(s) for k in t if k.startswith("dec_gemm.") for s in ("4x2", "1x6", "4x6", "5x6")), t
        for k in range(4):
            ref[k].append(logits[k])
    ref = [np.concatenate(r) for r in ref]
    logits, in_prompt, in_steps = _lane_run(E, ctx, lane, lane_pcm, 0, W.LANE_ROWS)
    print(f"width {d} lane of {W.LANE_ROWS} rows on {W.LANE_CUS} CUs: prompt pass {_short(in_prompt)}; steps {_short(in_steps)}")
    for n_new, tally, calls in ((2, in_prompt, 1), (1, in_steps, 3)):
        want = W.lane_shapes(d, n_new)
        for g in W.LANE_GEMMS:
            got = {k: v for k, v in tally.items() if k.startswith(f"dec_gemm.{g}.")}
            assert got == {W.counter_name(g, want[g]): calls * N_LAYER}, (d, n_new, g, got, want[g])
            _lane_seen.add(want[g])
    for k in range(4):
        assert np.isfinite(logits[k]).all()
        assert np.array_equal(logits[k].view(np.uint32), ref[k].view(np.uint32)), (d, k)
    lane.close()
    ctx.close()
    if d == W.LANE_WIDTHS[-1]:
        assert _lane_seen >= {"4x6", "4x2", "1x6", "1x2"}, _lane_seen


# ---------------------------------------------------------------------------------------------------------------------
# (d) kernel level
# ---------------------------------------------------------------------------------------------------------------------
def _td(dt):
    return torch.bfloat16 if dt == 0 else torch.float16


def _dev(a, td=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device="cuda", dtype=td)


def _stream():
    return torch.cuda.current_stream().cuda_stream


LN_WIDTHS = (512, 516, 768, 1024, 1028, 1152, 1284)      # MAXV 2 | 4 at 512 | 516, 4 | 5 at 1024 | 1028, 5 | 8 at 1280 | 1284


@pytest.mark.parametrize("dt", [0, 1], ids=["bf16", "f16"])
@pytest.mark.parametrize("tiled", [0, 1])
@pytest.mark.parametrize("d", LN_WIDTHS)
def test_layernorm_on_both_sides_of_every_instantiation(E, d, tiled, dt):
    """test_gpu_dec_gemm.py::test_layernorm_launch's check at the widths its list (64, 384, 1280, 2048) leaves out"""
    if tiled and d % 32 != 0:
        buf = torch.zeros(64, device="cuda")
        p = buf.data_ptr()
        assert E.lib().ohw_dbg_layernorm(dt, p, p, p, p, 1, d, 1, None) == E.OHW_E_INVALID_ARG      # refused before any launch
        return
    td = _td(dt)
    worst = 0.0
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
        dx = _dev(np.concatenate([x, np.full((R.GUARD_ROWS, d), np.nan)]))
        dg, db = _dev(gamma), _dev(beta)
        out = _dev(np.full(want.shape, R.SENTINEL), td)
        rc = E.lib().ohw_dbg_layernorm(dt, dx.data_ptr(), dg.data_ptr(), db.data_ptr(), out.data_ptr(), rows, d, tiled, _stream())
        assert rc == 0, E.last_error()
        torch.cuda.synchronize()
        err = np.abs(out.double().cpu().numpy() - want)
        assert (err <= lim).all(), (d, rows, float((err / np.maximum(lim, 1e-300)).max()))
        worst = max(worst, float((err[lim > 0] / lim[lim > 0]).max()))
    print(f"layernorm d {d} tiled {tiled} {DT_NAME[dt]}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("dt", [0, 1], ids=["bf16", "f16"])
@pytest.mark.parametrize("d", [512, 1024])
def test_embedding_at_base_and_medium_width(E, d, dt):
    """test_gpu_dec_gemm.py's embedding check: x = token row + position row in ONE fp32 addition, bit for bit; the 16-bit tiled
    copy and the per-16-column statistics within producer_expect's bound; sentinels behind the last row"""
    td = _td(dt)
    rng = np.random.default_rng([d, dt])
    M, n_new, V, P = 21, 3, 50, 16
    tok = np.array([0, 17, 33, 49, 15, 16, 31, 32, 48, 1, 47, 2, 18, 34, 49, 0, 20, 40, 5, 25, 45], dtype=np.int32)
    past = np.array([0, 13, 5, 2, 9, 13, 7], dtype=np.int32)                 # 13 + 3 == P
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
    want_x = emb[tok].astype(np.float32) + pos[rows]
    got_x = x.cpu().numpy()
    assert (got_x[:M].view(np.uint32) == want_x.view(np.uint32)).all() and (got_x[M:] == R.SENTINEL).all()
    c = R.case(R.RESID, R.PLAIN, M, d, d, stat=True)
    w16, st, st_lim = R.producer_expect(c, got_x[:M].astype(np.float64), dt)
    words = x16.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    assert (words == R.bits_T(w16, dt)).all()
    got = stat.double().cpu().numpy()
    ratio = np.abs(got[:M] - st) / st_lim
    print(f"embed d {d} {DT_NAME[dt]}: statistics worst error / bound {ratio.max():.3f}")
    assert (ratio <= 1.0).all() and (got[M:] == R.SENTINEL).all()


def _untile(out, M, d):
    idx = torch.from_numpy(A.act_tiled_index(M, d)).cuda()
    rest = torch.ones(out.numel(), dtype=torch.bool, device="cuda")
    rest[idx.reshape(-1)] = False
    return out[idx].double().cpu().numpy(), out[rest]


def _ndev(a, td):
    return torch.from_numpy(np.array(a)).to(device="cuda", dtype=td)      # a copy: the cases are read-only


def _needle_report(what, H, pattern, dt, err):
    print(f"needles {what} H {H} {pattern} {DT_NAME[dt]}: worst error {err:.3e} = {err / A.TOL[dt]:.3f} tol")


@pytest.mark.parametrize("dt", [0, 1], ids=["bf16", "f16"])
@pytest.mark.parametrize("H", W.NEEDLE_HEADS)
@pytest.mark.parametrize("slots", [False, True], ids=["plain", "slots"])
def test_self_attention_needles_at_real_head_counts(E, slots, H, dt):
    td = _td(dt)
    M, d = len(A.N_PAST), 64 * H
    n_past = np.ascontiguousarray(A.N_PAST, dtype=np.int32)
    for pattern in A.PATTERNS:
        c, ref, _ = W.needle_case("self", "slots" if slots else "plain", pattern, H)
        q, kc, vc = _ndev(c.q.reshape(M, d), td), _ndev(c.K, td), _ndev(c.V, td)
        out = torch.full((A.tiled_elems(M, d),), A.SENTINEL, device="cuda", dtype=td)
        table = np.ascontiguousarray(c.table, dtype=np.int32) if slots else None
        variant = C.c_int(-1)
        rc = E.lib().ohw_dbg_self_attn(dt, q.data_ptr(), kc.data_ptr(), vc.data_ptr(), E._ip(n_past), out.data_ptr(), M, 1, H, A.N_CTX,
                                       E._ip(table) if slots else None, C.byref(variant), _stream())
        assert rc == 0, E.last_error()
        torch.cuda.synchronize()
        assert variant.value == (E.SA_SLOTS if slots else E.SA_PLAIN)
        got, rest = _untile(out, M, d)
        err = A.worst_error(got, ref)
        _needle_report("self " + ("slots" if slots else "plain"), H, pattern, dt, err)
        assert err <= A.TOL[dt], (pattern, err)
        assert (rest == A.SENTINEL).all()


@pytest.mark.parametrize("dt", [0, 1], ids=["bf16", "f16"])
@pytest.mark.parametrize("H", W.NEEDLE_HEADS)
@pytest.mark.parametrize("name", list(W.XA_NEEDLES))
def test_cross_attention_needles_at_real_head_counts(E, name, H, dt):
    td = _td(dt)
    M, t_len, kv_group, invariant = W.XA_NEEDLES[name]
    d = 64 * H
    variant_name, ks = W.xa_variant(name, H)
    for pattern in A.PATTERNS:
        c, ref, _ = W.needle_case("cross", name, pattern, H)
        q, xk, xv = _ndev(c.q.reshape(M, d), td), _ndev(c.K, td), _ndev(c.V, td)
        partials = torch.full((M * H * A.XA_MAX_SPLIT * 68,), float("nan"), device="cuda")
        tickets = torch.zeros(M * H, device="cuda", dtype=torch.int32)
        out = torch.full((A.tiled_elems(M, d),), A.SENTINEL, device="cuda", dtype=td)
        variant = C.c_int(-1)
        rc = E.lib().ohw_dbg_cross_attn(dt, q.data_ptr(), xk.data_ptr(), xv.data_ptr(), out.data_ptr(), M, 1, H, t_len, kv_group, int(invariant),
                                        None, None, partials.data_ptr(), tickets.data_ptr(), M, C.byref(variant), _stream())
        assert rc == 0, E.last_error()
        torch.cuda.synchronize()
        assert variant.value == getattr(E, "XA_" + variant_name.upper()), (name, H, variant.value, variant_name)
        assert not tickets.any()
        got, rest = _untile(out, M, d)
        err = A.worst_error(got, ref)
        _needle_report(f"cross {name} [{variant_name}, {ks} slices]", H, pattern, dt, err)
        assert err <= A.TOL[dt], (pattern, err)
        assert (rest == A.SENTINEL).all()


@pytest.mark.parametrize("dt", [0, 1], ids=["bf16", "f16"])
@pytest.mark.parametrize("H", W.NEEDLE_HEADS)
@pytest.mark.parametrize("n_q", list(W.CHUNK_NEEDLES))
def test_prefill_cross_attention_needles_at_real_head_counts(E, n_q, H, dt):
    td = _td(dt)
    n_win, t_len = W.CHUNK_NEEDLES[n_q]
    M, d = n_q * n_win, 64 * H
    for pattern in A.PATTERNS:
        c, ref, _ = W.needle_case("chunk", n_q, pattern, H)
        q, xk, xv = _ndev(c.q.reshape(M, d), td), _ndev(c.K, td), _ndev(c.V, td)
        out = torch.full((A.tiled_elems(M, d),), A.SENTINEL, device="cuda", dtype=td)
        E.State.dbg_cross_attn_chunk(dt, q.data_ptr(), xk.data_ptr(), xv.data_ptr(), out.data_ptr(), n_win, H, t_len, stream=_stream(), n_q=n_q)
        torch.cuda.synchronize()
        got, rest = _untile(out, M, d)
        err = A.worst_error(got, ref)
        _needle_report(f"chunk n_q {n_q}", H, pattern, dt, err)
        assert err <= A.TOL[dt], (pattern, err)
        assert (rest == A.SENTINEL).all()


# ---------------------------------------------------------------------------------------------------------------------
# (e) the edge of what loads
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", W.TOO_WIDE)
def test_wider_models_are_refused_at_load(E, tmp_path, d):
    """the decoder's fused LayerNorm holds 1280 columns: a wider model would load, encode, and fail inside its first decode"""
    hp = W.shallow(d, n_layer=1)
    with pytest.raises(E.LoadFailed) as ei:
        E.Context.synthetic(hp, 1234, 0, E.OHW_DTYPE_F16)
    assert ei.value.code == E.OHW_E_LOAD_FAILED
    assert "n_text_state must be <= 1280" in str(ei.value), str(ei.value)
    path = str(tmp_path / f"ggml-w{d}.bin")
    modelfile.write_synthetic_model(path, synth.HParams(*hp), 1234)
    try:
        with pytest.raises(E.LoadFailed) as ei:
            E.Context.from_file(path, 0, E.OHW_DTYPE_F16)
    finally:
        os.remove(path)                                                  # a quarter to half a gigabyte
    assert ei.value.code == E.OHW_E_LOAD_FAILED
    assert "n_text_state must be <= 1280" in str(ei.value), str(ei.value)


@pytest.mark.parametrize("dt", [1, 0], ids=["f16", "bf16"])
def test_the_widest_model_loads_with_one_layer_and_matches(E, oracle, pcm, dt):
    _, _, same, total, _ = _whole_path(E, oracle, pcm, W.shallow(W.MAX_WIDTH, n_layer=1), dt)
    assert total == 76
