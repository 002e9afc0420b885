"""LN1 + QKV and LN2 + mlp.0 for many rows on few CUs: the LayerNorm once as a launch of its own (dec_ln_rows_kernel) and a
GEMM whose workgroups hold four or five n-tiles of weights for all rows (dec_gemm_rows_kernel, shapes 4x6 / 5x6), against the
fused forms they stand in for.  Both promise dec_gemm_kernel's arithmetic in dec_gemm_kernel's order, so the comparison has
no tolerance: raw words.  Which kernel ran is asserted every time (shape_out, ohw_dbg_counter).

The pick rule (dec_gemm_pick, decode.hip), with mt = ceil(M / 16), nt = ceil(N / 16), cus = cu_budget: ln form, QKV or GELU_T,
mt > 2, ceil(nt / 4) * ceil(mt / 2) > 2 cus, and the all-rows grid ceil(nt / NTW) >= 32; NTW = 4, for GELU_T 5 when
ceil(nt / 4) > cus.  At cu_budget = 32:
  QKV     N = 2112 (132 n-tiles)  33 * ceil(mt / 2) > 64 from mt = 3 on: 4x6 for every M below
  GELU_T  N = 2048 (128 n-tiles)  32 * ceil(mt / 2) > 64 needs mt >= 5: 4x6 at M = 95, 96, 100; M = 33 and 40 (mt = 3: 64
                                  workgroups, exactly two rounds) are NOT over two rounds and keep 4x2 - the rule as stated;
                                  those lines are still run, compared and bounded, and the M = 33 / 40 paths of the new kernel
                                  (a partial last m-tile, an empty second pass) are reached through QKV and the ragged lines
  GELU_T  N = 2016 (126 n-tiles)  NTW = 4, 32 workgroups: the last holds two real tiles of four
  GELU_T  N = 2528 (158 n-tiles)  40 > 32: NTW = 5, 32 workgroups: the last holds three real tiles of five; every M
"""
import numpy as np
import pytest

import dec_gemm_ref as R
from dec_gemm_ref import GELU_T, LN, QKV, S1x2, S4x2, case
from test_gpu_dec_gemm import _words, check, launch

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

S4x6, S5x6 = 6, 7            # kernels.hpp DecGemmShape, behind 1x6
SHAPE_NAMES = R.SHAPE_NAMES + ("4x6", "5x6")
CU = 32
NCTX = 12
MS = (33, 40, 95, 96, 100)   # a partial last m-tile; an empty m-tile (and pass) in a workgroup; a seventh m-tile in a second row group
KS = (64, 320, 1280)         # six waves without a k-block; a ragged share (10 blocks on 8 waves); all five blocks per wave


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from openhush_amd import engine
    engine.lib()
    return engine


def _qkv(M, K, n_new):
    B = M // n_new
    past = [(7 * b) % 13 for b in range(B)] if n_new == 1 else [(5 * b) % 13 for b in range(B)]     # 12 == n_ctx; 10 .. 12 + 3 pass it
    return case(QKV, LN, M, 2112, K, cu=CU, n_new=n_new, n_past=past, n_ctx=NCTX)


def _gelu_want(M):
    return S4x6 if (M + 15) // 16 >= 5 else S4x2


LINES = ([(case(GELU_T, LN, M, 2048, K, cu=CU), _gelu_want(M)) for M in MS for K in KS] +
         [(_qkv(M, K, 1), S4x6) for M in MS for K in KS] +
         [(_qkv(M, K, 3), S4x6) for M in (33, 96) for K in KS] +
         [(case(GELU_T, LN, 100, 2016, 320, cu=CU), S4x6)] +
         [(case(GELU_T, LN, M, 2528, 1280, cu=CU), S5x6) for M in MS])


def test_lines_follow_the_stated_rule():
    """the expectations above, recomputed from the rule's own words"""
    seen = set()
    for c, want in LINES:
        mt, nt = (c["M"] + 15) // 16, (c["N"] + 15) // 16
        over_two_rounds = mt > 2 and -(-nt // 4) * -(-mt // 2) > 2 * CU
        ntw = 5 if c["epi"] == GELU_T and -(-nt // 4) > CU else 4
        new = over_two_rounds and -(-nt // ntw) >= 32
        assert want == ((S4x6 if ntw == 4 else S5x6) if new else S4x2), R.case_name(c)
        seen.add((c["epi"], want))
    assert seen == {(GELU_T, S4x6), (GELU_T, S5x6), (GELU_T, S4x2), (QKV, S4x6)}


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("c,want", LINES, ids=[R.case_name(c) for c, _ in LINES])
def test_all_rows_form_gives_the_words_of_the_fused_form(E, c, want, dt):
    I = R.make(c, "real", dt)
    new, shape = launch(E, c, I, dt)
    assert shape == want, (R.case_name(c), SHAPE_NAMES[shape], SHAPE_NAMES[want])
    old, shape0 = launch(E, c, I, dt, cu=0)
    assert shape0 == S1x2, SHAPE_NAMES[shape0]
    for k in new:
        bad = np.argwhere(_words(new[k]) != _words(old[k]))
        assert len(bad) == 0, (R.case_name(c), k, len(bad), bad[:4].tolist())
    # float64 bounds, and the sentinel wherever the contract names nothing (guard rows, pad rows, positions past n_ctx)
    worst = check(c, I, dt, "real", new, f"{R.case_name(c)} dt {dt}")
    print(f"lane ln forms {R.case_name(c)} dt {dt} {SHAPE_NAMES[shape]}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("K", [320, 1280])
def test_layernorm_launch_keeps_the_summation_order(E, K, dt):
    """rows with a large mean against a small deviation: the fp32 row sum loses about seven of the deviation's bits, so a sum
    taken in another order gives another mean, other deviations and other 16-bit words.  Word equality only: the float64
    bound of dec_gemm_ref has no term for the cancellation, which both forms suffer alike"""
    c = case(GELU_T, LN, 95, 2048, K, cu=CU)
    I = R.make(c, "real", dt)
    rng = np.random.default_rng([K, dt, 95])
    I.x = (100.0 + 13.0 * np.arange(95)[:, None] + 0.05 * rng.standard_normal((95, K))).astype(np.float32).astype(np.float64)
    new, shape = launch(E, c, I, dt)
    assert shape == S4x6, SHAPE_NAMES[shape]
    old, shape0 = launch(E, c, I, dt, cu=0)
    assert shape0 == S1x2, SHAPE_NAMES[shape0]
    a, b = _words(new["out"]), _words(old["out"])
    assert len(np.unique(a)) > 1000                      # a real image, not a constant
    assert (a == b).all(), int((a != b).sum())


# ---- through ohw_decode -----------------------------------------------------------------------------------------------------
N_WIN = 96
LANE_CUS = 32
AUDIO_CTX = 64
# text width 768: QKV has 144 n-tiles (36 workgroups of four), mlp.0 192 (48 > 32 CUs: five per workgroup, 39 workgroups)
HP = [51865, 1500, 768, 12, 1, 448, 768, 12, 2, 80, 1]
N_LAYER = 2
NEW_QKV, NEW_FC1 = "dec_gemm.qkv.ln.4x6", "dec_gemm.fc1.ln.5x6"


def _decode_run(E, ctx, lane, pcm, first, count):
    """a two-token prompt pass and three single-token steps of windows first .. first + count - 1 as ONE batch on the lane
    stream -> (the four logits arrays, [qkv, fc1] launches of the new forms in the prompt pass, the same in the three steps)"""
    tok = ctx.tok
    prompt = np.asarray([tok.sot, tok.no_timestamps], np.int32)
    st = E.State(ctx, count)
    st.set_batch_invariant(True)
    st.set_stream(lane.ptr)
    st.set_audio_ctx(AUDIO_CTX)
    st.mel(pcm[first:first + count], None, E.OHW_MEL_ZERO_TAIL, want=False)
    st.encode(count)
    logits = [st.decode(np.tile(prompt, (count, 1)), [0] * count)]
    in_prompt = [st.counter(NEW_QKV), st.counter(NEW_FC1)]
    for i in range(3):
        logits.append(st.decode(logits[-1].argmax(axis=1).astype(np.int32)[:, None], [2 + i] * count))
    in_steps = [st.counter(NEW_QKV) - in_prompt[0], st.counter(NEW_FC1) - in_prompt[1]]
    st.close()
    return logits, in_prompt, in_steps


@pytest.fixture(scope="module")
def wide_lane(E):
    """the reference, computed once and left unchanged: the 96 windows in batches of 16 on the 32-CU stream.  A 16-row batch
    has one m-tile in a step and two in its two-token prompt pass: the fused forms, every time"""
    from openhush_amd import synth
    ctx = E.Context.synthetic(HP, 4321, 0, E.OHW_DTYPE_BF16)
    lane = E.Stream(0, 0, LANE_CUS)
    pcm = np.stack([synth.synth_audio(900 + w, AUDIO_CTX * 320) for w in range(N_WIN)])
    ref = [[] for _ in range(4)]
    for f in range(0, N_WIN, 16):
        logits, in_prompt, in_steps = _decode_run(E, ctx, lane, pcm, f, 16)
        assert in_prompt == [0, 0] and in_steps == [0, 0], (in_prompt, in_steps)
        for k in range(4):
            ref[k].append(logits[k])
    ref = [np.concatenate(r) for r in ref]
    for r in ref:
        r.setflags(write=False)
    yield ctx, lane, pcm, ref
    lane.close()
    ctx.close()


@pytest.mark.parametrize("rows", [96, 33, 95])
def test_decode_with_the_all_rows_forms_gives_the_bits_of_the_16_row_batches(E, wide_lane, rows):
    """one `rows`-row batch against the same windows in batches of 16: prompt pass and three single-token steps, logits bit for
    bit; the new forms ran for QKV and mlp.0 in every layer of every pass"""
    ctx, lane, pcm, ref = wide_lane
    logits, in_prompt, in_steps = _decode_run(E, ctx, lane, pcm, 0, rows)
    print(f"rows {rows}: all-rows launches [qkv, fc1] {in_prompt} (prompt) + {in_steps} (steps)")
    assert in_prompt == [N_LAYER, N_LAYER] and in_steps == [3 * N_LAYER, 3 * N_LAYER]
    for k in range(4):
        assert np.array_equal(logits[k].view(np.uint32), ref[k][:rows].view(np.uint32)), (rows, k)
