"""mlp.2 with up to six m-tiles per workgroup (dec_gemm_rows_kernel, the form a decode picks for many rows on few CUs: a
lane of the LANES schedule) against the kernels it stands in for, bit for bit, through ohw_decode on a 16-CU stream.  The
kernel promises dec_gemm_kernel's arithmetic in dec_gemm_kernel's order, so there is no tolerance: the raw words of the
logits are compared.  Which kernel ran is asserted (ohw_dbg_counter): a test that takes the old path twice proves nothing.

"tiny" dims: d = 384, so mlp.2 has K = 1536 > 1280 and 24 n-tiles; on 16 CUs the two-m-tile grid (24 x ceil(m-tiles / 2))
exceeds the 32 slots from three m-tiles (33 rows) on.  A 16-row single-token step has one m-tile and keeps the old kernels;
its prompt pass is a 64-row launch (16 windows x 4 prompt tokens) and meets the rows rule like any other 64-row launch - the
rule knows rows and CUs, not batches - so the 16-row reference is asserted step by step.

(The LDS-staged self-attention the same change tried is not here: it measured no gain and was removed, DESIGN.md Appendix A.)
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N_WIN = 96
LANE_CUS = 16
NEW_SHAPE = "dec_gemm.fc2.1x6"


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from openhush_amd import engine
    engine.lib()
    return engine


def _decode_run(E, ctx, lane, pcm, first, count):
    """prompt pass and three single-token steps of windows first .. first + count - 1 as ONE batch on the lane stream ->
    (the four logits arrays, mlp.2 launches of the rows kernel in the prompt pass, the same in the three steps)"""
    tok = ctx.tok
    prompt = np.asarray([tok.sot, tok.sot + 1, tok.transcribe, tok.no_timestamps], np.int32)
    st = E.State(ctx, count)
    st.set_batch_invariant(True)
    st.set_stream(lane.ptr)
    st.mel(pcm[first:first + count], None, E.OHW_MEL_ZERO_TAIL, want=False)
    st.encode(count)
    logits = [st.decode(np.tile(prompt, (count, 1)), [0] * count)]
    in_prompt = st.counter(NEW_SHAPE)
    for i in range(3):
        logits.append(st.decode(logits[-1].argmax(axis=1).astype(np.int32)[:, None], [4 + i] * count))
    in_steps = st.counter(NEW_SHAPE) - in_prompt
    st.close()
    return logits, in_prompt, in_steps


@pytest.fixture(scope="module")
def tiny_lane(E):
    """the reference, computed once and left unchanged: the 96 windows in batches of 16 on the 16-CU stream"""
    from openhush_amd import synth
    hp = synth.PRESETS["tiny"]
    ctx = E.Context.synthetic(hp.as_list(), 1234, 0, E.OHW_DTYPE_BF16)
    lane = E.Stream(0, 0, LANE_CUS)
    pcm = np.stack([synth.synth_audio(500 + w, 64000) for w in range(N_WIN)])
    ref = [[] for _ in range(4)]
    for f in range(0, N_WIN, 16):
        logits, in_prompt, in_steps = _decode_run(E, ctx, lane, pcm, f, 16)
        assert in_steps == 0, in_steps                    # 16 rows: today's kernels in every single-token step
        assert in_prompt == hp.n_text_layer, in_prompt    # 64 rows: chosen by rows, as for any batch
        for k in range(4):
            ref[k].append(logits[k])
    ref = [np.concatenate(r) for r in ref]
    for r in ref:
        r.setflags(write=False)
    yield ctx, lane, pcm, ref, hp
    lane.close()
    ctx.close()


@pytest.mark.parametrize("rows", [96, 40, 33, 95])
def test_mlp2_rows_form_gives_the_bits_of_the_16_row_batches(E, tiny_lane, rows):
    """one `rows`-row batch against the same windows in batches of 16: prompt pass and three single-token steps, logits bit for
    bit.  33 and 95 leave a partial last m-tile (clamped, masked rows: they must neither fault nor store); 40 and 33 leave
    whole m-tiles of a workgroup empty"""
    ctx, lane, pcm, ref, hp = tiny_lane
    logits, in_prompt, in_steps = _decode_run(E, ctx, lane, pcm, 0, rows)
    print(f"rows {rows}: rows-kernel launches {in_prompt} (prompt) + {in_steps} (steps)")
    assert in_prompt == hp.n_text_layer and in_steps == 3 * hp.n_text_layer      # the new shape did run, in every layer
    for k in range(4):
        assert np.array_equal(logits[k].view(np.uint32), ref[k][:rows].view(np.uint32)), (rows, k)
