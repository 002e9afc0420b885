"""The prefill in 16-position chunks (ohw_state_set_prefill_chunk(16)): the decoder step at n_new = 16 and
cross_attn_chunk_kernel<T, 16, VAR> under a context table.  The oracle is fed the GPU's encoder output and the whole sequence at
position 0, as in test_gpu_prompt.py, whose tolerance (TOL_LOGIT) and pick rule are used unchanged.

Context lengths [0, 1, 15, 16, 17, 37] tokens occupy 0, 2, 16, 17, 18 and 38 positions: none, a chunk with 14 surplus rows, exactly
one chunk, one row into the second chunk, and three chunks with a ragged last one.
"""
import numpy as np
import pytest

import test_gpu_carry as TC
import test_gpu_long_batch as LB
import test_gpu_prompt as P
from test_gpu_long_batch import oracle_tokens, recs  # noqa: F401 - fixtures
from test_gpu_prompt import E, oracle  # noqa: F401 - fixtures
from openhush_amd import synth

pytestmark = pytest.mark.gpu

CTX_LENS = [0, 1, 15, 16, 17, 37]
TOL_LOGIT = P.TOL_LOGIT


def _state16(E, preset, dt, B, mode, pcm=None, chunk=16):
    assert hasattr(E.lib(), "ohw_state_set_prefill_chunk")
    ctx, st = P._state(E, preset, dt, B, mode, pcm=pcm)
    st.set_prefill_chunk(chunk)
    assert st.prefill_chunk() == chunk
    return ctx, st


def _prompt(tok):
    return [tok.sot, tok.sot + 1, tok.transcribe, tok.timestamp_begin]


@pytest.mark.parametrize("preset,dt,mode", [("micro", 0, "invariant"), ("micro", 1, "invariant"), ("micro-v3", 0, "invariant"),
                                            ("micro-v3", 1, "invariant"), ("micro", 1, "plain"), ("micro", 1, "var")])
def test_logits_behind_a_context_match_the_oracle_at_chunk_16(E, oracle, preset, dt, mode):
    B = len(CTX_LENS)
    ctx, st = _state16(E, preset, dt, B, mode)
    hp = synth.PRESETS[preset]
    om = oracle.Model.synth(hp.as_list(), 1234)
    tok = ctx.tok
    ctxs = P._contexts(tok, CTX_LENS)
    enc = st.fetch("enc", B)
    st.set_window_prompt(ctxs)
    lens = [st.window_prompt_len(b) for b in range(B)]
    assert lens == [0 if n == 0 else n + 1 for n in CTX_LENS]
    seqs, refs = [], []
    for b in range(B):
        seq = ([tok.prev] + ctxs[b] if ctxs[b] else []) + _prompt(tok) + P._forced(tok, 100 + b)
        s = oracle.State(om)
        s.set_encoder_output(enc[b])
        refs.append(s.decode(seq, 0, all_pos=True))
        seqs.append(seq)
    before = st.counter("xattn.chunk")
    st.prefill(B)
    chunks = st.counter("xattn.chunk") - before
    # 38 positions are 3 chunks of 16; 6 windows x 4 heads < 256: the chunk kernel needs the invariant or the per-window mode
    assert chunks == (3 * hp.n_text_layer if mode in ("invariant", "var") else 0), (mode, chunks)
    tol, worst = TOL_LOGIT[dt], 0.0
    lg = st.decode(np.asarray([s[n:n + 4] for s, n in zip(seqs, lens)], np.int32), lens)
    for b in range(B):
        worst = max(worst, P._check_row(lg[b], refs[b][lens[b] + 3], tol, (mode, b, "prompt")))
    for i in range(P.N_FORCED):
        pos = [n + 4 + i for n in lens]
        lg = st.decode(np.asarray([[s[p]] for s, p in zip(seqs, pos)], np.int32), pos)
        for b in range(B):
            worst = max(worst, P._check_row(lg[b], refs[b][pos[b]], tol, (mode, b, i)))
    print(f"chunk 16 logits {preset} dtype {dt} {mode}: worst error {worst:.4f} (tol {tol})")
    om.close()


def _logits(st, tok, B, lens):
    st.prefill(B)
    a = st.decode(np.asarray([_prompt(tok)] * B, np.int32), lens).copy()
    b = st.decode(np.asarray([[7]] * B, np.int32), [n + 4 for n in lens]).copy()
    return a, b


@pytest.mark.parametrize("dt", [0, 1])
def test_chunk_16_against_chunk_8_and_back(E, dt):
    """one state, one table: chunk 16 agrees with chunk 8 within the logit tolerance (the GEMMs see 16 rows per window instead of
    8, so bit equality is not required: printed); 12 is refused and changes nothing; back at 8 the first logits come again, bit
    for bit - the table was laid out again each time"""
    B = len(CTX_LENS)
    ctx, st = _state16(E, "micro", dt, B, "invariant", chunk=8)
    tok = ctx.tok
    st.set_window_prompt(P._contexts(tok, CTX_LENS))
    lens = [st.window_prompt_len(b) for b in range(B)]
    a8, b8 = _logits(st, tok, B, lens)
    st.set_prefill_chunk(16)
    a16, b16 = _logits(st, tok, B, lens)
    with pytest.raises(E.WhisperError) as ex:
        st.set_prefill_chunk(12)
    assert ex.value.code == E.OHW_E_INVALID_ARG and st.prefill_chunk() == 16
    for bad in (0, 4, 32, -16):
        with pytest.raises(E.WhisperError):
            st.set_prefill_chunk(bad)
    diff = max(float(np.abs(a16 - a8).max()), float(np.abs(b16 - b8).max()))
    equal = [bool(np.array_equal(a16[b], a8[b]) and np.array_equal(b16[b], b8[b])) for b in range(B)]
    print(f"chunk 16 against chunk 8, dtype {dt}: largest logit difference {diff:.3e} (tol {TOL_LOGIT[dt]}), rows bit-equal {equal}")
    assert diff < TOL_LOGIT[dt]
    assert equal[0]                                   # no context: no prefill at either size
    st.set_prefill_chunk(8)
    a8b, b8b = _logits(st, tok, B, lens)
    assert np.array_equal(a8b, a8) and np.array_equal(b8b, b8)
    # a table set while the size is 16, read at 8
    st.set_prefill_chunk(16)
    st.set_window_prompt(P._contexts(tok, CTX_LENS))
    st.set_prefill_chunk(8)
    a8c, b8c = _logits(st, tok, B, lens)
    assert np.array_equal(a8c, a8) and np.array_equal(b8c, b8)


def test_a_window_does_not_depend_on_its_batch_at_chunk_16(E):
    """test_gpu_prompt's statement at chunk 16: the window with 17 context tokens gives the same bits alone and in the batch of 6;
    the window without context gives the bits of a state with no table"""
    B, dt = len(CTX_LENS), 1
    ctx, st = _state16(E, "micro", dt, B, "invariant")
    tok = ctx.tok
    ctxs = P._contexts(tok, CTX_LENS)
    st.set_window_prompt(ctxs)
    lens = [st.window_prompt_len(b) for b in range(B)]
    full, nxt = _logits(st, tok, B, lens)
    pcm = P._pcm(B)
    for w in (4, 5, 1):
        _, one = _state16(E, "micro", dt, 1, "invariant", pcm=pcm[w:w + 1])
        one.set_window_prompt([ctxs[w]])
        a, b = _logits(one, tok, 1, [lens[w]])
        assert np.array_equal(a[0], full[w]) and np.array_equal(b[0], nxt[w]), w
    _, bare = _state16(E, "micro", dt, 1, "invariant", pcm=pcm[0:1])
    a, b = _logits(bare, tok, 1, [0])                  # no table: the prefill is a no-op
    assert np.array_equal(a[0], full[0]) and np.array_equal(b[0], nxt[0])


def test_carry_at_chunk_16_long_batch_equals_alone(E, recs, oracle_tokens, tmp_models):
    eng = TC._engine(E, tmp_models("micro"), oracle_tokens)
    eng.set_carry_context()
    base = TC._alone(E, eng, recs[1])
    eng.set_prefill_chunk(16)
    with pytest.raises(E.WhisperError):
        eng.set_prefill_chunk(12)
    alone = [TC._alone(E, eng, p) for p in recs]
    LB._check_lone_runs_make_it_a_test(alone, LB.MAX_BATCH)
    assert any(len(c) > 16 for a in alone for c in a["contexts"])            # some context spans more than one chunk
    for a in alone:
        assert a["contexts"] == TC._expected(a)
    together = TC._together(E, eng, recs)
    for i in range(len(recs)):
        assert together[i]["tokens"] == alone[i]["tokens"], i
        assert together[i] == alone[i], i
    print(f"\ncarry at chunk 16 against chunk 8, 75 s recording: tokens equal {alone[1]['tokens'] == base['tokens']}")
    eng.set_prefill_chunk(8)
    assert TC._alone(E, eng, recs[1]) == base
    eng.close()
