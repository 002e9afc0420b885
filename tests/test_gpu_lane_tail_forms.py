"""The logits of a lane's token step (96 rows on 64 CUs: a lane of the LANES schedule) in their all-rows form, against the form
they stand in for: dec_gemm_rows_kernel's held-weights body with the LOGITS epilogue (shape 4x6).  A workgroup requests its
four n-tiles of the embedding once and runs two passes of three m-tiles over all rows; dec_gemm_kernel<LOGITS, 4, 2> requests
them once per 32-row block.

The form promises dec_gemm_kernel's arithmetic in dec_gemm_kernel's order per (m-tile, n-tile), so the comparison with the same
case at cu_budget = 0 (which picks the present form) has no tolerance: raw words.  Which kernel ran is asserted every time.

The pick rule (dec_gemm_pick, decode.hip), with mt = ceil(M / 16), nt = ceil(N / 16), cus = cu_budget:
  logits  cu_budget > 0 (a CU-masked stream), mt > 2, K <= 1280, nt * ceil(mt / 2) > 2 cus, and the all-rows grid
          ceil(nt / 4) has at least 32 workgroups and at most 16 rounds of cus: 4x6; else 4x2 under the first four conditions
At cu_budget = 4:
  N = 2010 = 16 * 125 + 10 (126 n-tiles, the last with ten columns): 32 workgroups, the last holds two tiles of four

The two-n-tile form of mlp.2 and the four-tile cross query that were measured with this form did not reach their bar and are
not in the tree: they have no tests here.
"""
import numpy as np
import pytest

import dec_gemm_ref as R
from dec_gemm_ref import LOGITS, PLAIN, S2x2, S4x2, case
from test_gpu_dec_gemm import _words, check, launch

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

S4x6, S5x6 = 6, 7            # kernels.hpp DecGemmShape, behind 1x6
SHAPE_NAMES = R.SHAPE_NAMES + ("4x6", "5x6")
CU = 4
MS = (33, 48, 96, 100)       # a last m-tile with one row; a pass without rows; all six tiles; a ragged seventh in a second row group
KS = (64, 384, 1280)         # fewer k-blocks than waves; a ragged share (12 blocks on 8 waves); all five blocks per wave
N_LOGITS, LD_LOGITS = 2010, 2024

LOGIT_LINES = ([(case(LOGITS, PLAIN, M, N_LOGITS, K, cu=CU, ld=LD_LOGITS), S4x6, S2x2) for M in MS for K in KS] +
               [(case(LOGITS, PLAIN, M, N_LOGITS, K, cu=CU, n_new=3, ld=LD_LOGITS), S4x6, S2x2) for M in (33, 48, 96) for K in KS])
# lines that must stay where they are: a grid below 32 workgroups, a stream narrower than a 16th of the grid, the whole chip,
# two m-tiles
KEPT_LINES = [(case(LOGITS, PLAIN, 96, 16 * 124, 384, cu=CU), S4x2, None),          # 31 workgroups
              (case(LOGITS, PLAIN, 96, 16 * 260, 384, cu=CU), S4x2, None),          # 65 workgroups: over 16 rounds of 4 CUs
              (case(LOGITS, PLAIN, 96, N_LOGITS, 384, cu=0), S2x2, None),
              (case(LOGITS, PLAIN, 32, N_LOGITS, 384, cu=CU), S2x2, None)]
LINES = LOGIT_LINES


def _rule(c):
    """the pick rules of the module docstring, from their own words"""
    mt, nt = -(-c["M"] // 16), -(-c["N"] // 16)
    cus = c["cu"] if c["cu"] > 0 else 256
    half_m = -(-mt // 2)
    assert c["epi"] == LOGITS
    if mt == 1:
        return R.S2x1
    if mt > 2 and c["K"] <= 1280 and nt * half_m > 2 * cus:
        g4 = -(-nt // 4)
        return S4x6 if c["cu"] > 0 and 32 <= g4 <= 16 * cus else S4x2
    return S2x2


def test_lines_follow_the_stated_rule():
    seen = set()
    for c, want, want0 in LINES + KEPT_LINES:
        assert want == _rule(c), R.case_name(c)
        if want0 is not None:
            assert want0 == _rule(dict(c, cu=0)), R.case_name(c)
        seen.add((c["epi"], want))
    assert seen == {(LOGITS, S4x6), (LOGITS, S4x2), (LOGITS, S2x2)}
    # the last workgroup is ragged as the docstring says
    assert N_LOGITS % 16 == 10 and -(-N_LOGITS // 16) % 4 == 2


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from openhush_amd import engine
    engine.lib()
    return engine


@pytest.mark.parametrize("c,want,_w0", KEPT_LINES, ids=[R.case_name(c) for c, _, _ in KEPT_LINES])
def test_lines_outside_the_rules_keep_their_kernel(E, c, want, _w0):
    I = R.make(c, "real", 0)
    out, shape = launch(E, c, I, 0)
    assert shape == want, (R.case_name(c), SHAPE_NAMES[shape], SHAPE_NAMES[want])
    check(c, I, 0, "real", out, R.case_name(c))


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("c,want,want0", LINES, ids=[R.case_name(c) for c, _, _ in LINES])
def test_all_rows_form_gives_the_words_of_the_present_form(E, c, want, want0, dt):
    I = R.make(c, "real", dt)
    new, shape = launch(E, c, I, dt)
    assert shape == want, (R.case_name(c), SHAPE_NAMES[shape], SHAPE_NAMES[want])
    old, shape0 = launch(E, c, I, dt, cu=0)
    assert shape0 == want0, SHAPE_NAMES[shape0]
    a, b = _words(new["out"]), _words(old["out"])
    bad = np.argwhere(a != b)
    assert len(bad) == 0, (R.case_name(c), len(bad), bad[:4].tolist())
    # what the contract does not name still holds the sentinel: the columns N .. ld - 1 of every row (the six columns the last
    # n-tile does not have, and the pad) and the rows of windows that do not exist
    got = new["out"].double().cpu().numpy()
    rows = c["M"] // c["n_new"]
    assert (got[:, c["N"]:] == R.SENTINEL).all() and (got[rows:] == R.SENTINEL).all()
    assert len(np.unique(a[:rows, :c["N"]])) > 1000             # a real image was written
    # float64 bounds (and the sentinel again, element by element)
    worst = check(c, I, dt, "real", new, f"{R.case_name(c)} dt {dt}")
    print(f"lane tail forms {R.case_name(c)} dt {dt} {SHAPE_NAMES[shape]}: worst error / bound {worst:.3f}")


# ---- through ohw_decode -----------------------------------------------------------------------------------------------------
N_WIN = 96
LANE_CUS = 64
AUDIO_CTX = 64
NEW_LOGITS = "dec_gemm.logits.4x6"


def _decode_run(E, ctx, lane, pcm, first, count):
    """a two-token prompt pass and three single-token steps of windows first .. first + count - 1 as ONE batch on the lane
    stream -> (the four logits arrays, logits launches of the all-rows form)"""
    tok = ctx.tok
    prompt = np.asarray([tok.sot, tok.no_timestamps], np.int32)
    st = E.State(ctx, count)
    st.set_batch_invariant(True)
    st.set_stream(lane.ptr)
    st.set_audio_ctx(AUDIO_CTX)
    st.mel(pcm[first:first + count], None, E.OHW_MEL_ZERO_TAIL, want=False)
    st.encode(count)
    logits = [st.decode(np.tile(prompt, (count, 1)), [0] * count)]
    for i in range(3):
        logits.append(st.decode(logits[-1].argmax(axis=1).astype(np.int32)[:, None], [2 + i] * count))
    n = st.counter(NEW_LOGITS)
    st.close()
    return logits, n


@pytest.fixture(scope="module")
def tiny_lane(E):
    """the reference, computed once and left unchanged: the 96 windows in batches of 16 on the 64-CU stream.  A 16-row batch has
    one m-tile in a step and two in its two-token prompt pass: never the all-rows form"""
    from openhush_amd import synth
    ctx = E.Context.synthetic(synth.PRESETS["tiny"].as_list(), 4321, 0, E.OHW_DTYPE_BF16)
    lane = E.Stream(0, 0, LANE_CUS)
    pcm = np.stack([synth.synth_audio(900 + w, AUDIO_CTX * 320) for w in range(N_WIN)])
    ref = [[] for _ in range(4)]
    for f in range(0, N_WIN, 16):
        logits, n = _decode_run(E, ctx, lane, pcm, f, 16)
        assert n == 0, n
        for k in range(4):
            ref[k].append(logits[k])
    ref = [np.concatenate(r) for r in ref]
    for r in ref:
        r.setflags(write=False)
    yield ctx, lane, pcm, ref
    lane.close()
    ctx.close()


@pytest.mark.parametrize("rows", [96, 33, 95])
def test_decode_with_the_all_rows_logits_gives_the_bits_of_the_16_row_batches(E, tiny_lane, rows):
    """one `rows`-row batch against the same windows in batches of 16: prompt pass (n_new = 2: every second row is stored) and
    three single-token steps, logits bit for bit; the all-rows form ran in every call"""
    ctx, lane, pcm, ref = tiny_lane
    logits, n = _decode_run(E, ctx, lane, pcm, 0, rows)
    assert n == 4, n
    for k in range(4):
        assert np.array_equal(logits[k].view(np.uint32), ref[k][:rows].view(np.uint32)), (rows, k)
