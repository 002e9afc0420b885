"""Packed-row encoder (ohw_state_set_packed_encoder) on the GPU: under per-window lengths the encoder runs on sum(n_ctx) rows,
the windows laid end to end, and everything behind it is unchanged.

The stages are row-wise and the packed attention keeps the reduction order of the unpacked one, so the requirement is equality
by bits with the unpacked ragged path - of the valid rows of the encoder taps and the cross K/V, and of tokens and token
log-probabilities.  There is no tolerance in this file.

The lengths put window starts off every 64-, 128- and 256-row tile and query-block boundary, include a one-row window and a
window shorter than a key block, and sum to no tile multiple (648 and 2026 rows).
"""
import numpy as np
import pytest

from openhush_amd import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MICRO = synth.PRESETS["micro"]
MIXES = {256: [256, 64, 130, 1, 197], 1500: [1500, 128, 321, 77]}
WHATS = ("enc", "block0", "xk0", "xv1")


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from openhush_amd import engine
    engine.lib()
    assert hasattr(engine.lib(), "ohw_state_set_packed_encoder")
    return engine


@pytest.fixture(scope="module")
def ctxs(E):
    return {dt: E.Context.synthetic(MICRO.as_list(), 1234, 0, dt) for dt in (0, 1)}


def _pcm_batch():
    b = np.zeros(synth.CHUNK_SAMPLES, np.float32)
    b[:48000] = synth.synth_audio(3, 48000)
    return (np.stack([synth.synth_audio(7), b, synth.synth_audio(11), synth.synth_audio(13), synth.synth_audio(17)]),
            [synth.CHUNK_SAMPLES, 48000, synth.CHUNK_SAMPLES, synth.CHUNK_SAMPLES, synth.CHUNK_SAMPLES])


PCM, NS = _pcm_batch()


def _run_mix(E, st, env, lens, first=0):
    B = len(lens)
    st.set_audio_ctx(env)
    st.set_window_ctx(lens)
    st.mel(PCM[first:first + B], NS[first:first + B], E.OHW_MEL_ZERO_TAIL, want=False)
    st.encode(B)


def _valid(st, what, lens):
    a = st.fetch(what, len(lens))
    return [a[b, :n].copy() for b, n in enumerate(lens)]


def _walk(ctx, st, B):
    p = ctx.default_params()
    p.force_len = 8
    return st.greedy_ex(B, p)


def _same_walk(x, y):
    return len(x["tokens"]) == 8 and x["tokens"] == y["tokens"] and np.array_equal(x["logprobs"], y["logprobs"])


def _rows_equal(x, y):
    return x.shape == y.shape and not np.isnan(x).any() and np.array_equal(x, y)


@pytest.fixture(scope="module")
def unpacked(E, ctxs):
    """the unpacked ragged run of every (dtype, envelope): valid rows and the forced greedy walk - computed once, never changed"""
    ref = {}
    for dt in (0, 1):
        for env, lens in MIXES.items():
            st = E.State(ctxs[dt], len(lens))
            assert not st.packed_encoder                         # the default
            _run_mix(E, st, env, lens)
            assert st.counter("enc_rows") == len(lens) * env
            ref[dt, env] = ({w: _valid(st, w, lens) for w in WHATS + ("stem",)}, _walk(ctxs[dt], st, len(lens)))
            st.close()
    return ref


# 1. bit equality with the unpacked ragged path, on the same state, and with every window run alone
@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("env", [256, 1500])
def test_packed_rows_carry_the_bits_of_the_unpacked_run(E, ctxs, unpacked, dt, env):
    ctx, lens = ctxs[dt], MIXES[env]
    B = len(lens)
    st = E.State(ctx, B)
    _run_mix(E, st, env, lens)                                   # switch off, then on: the same state, mel and lengths
    off = {w: _valid(st, w, lens) for w in WHATS}
    off_walk = _walk(ctx, st, B)
    st.set_packed_encoder(True)
    assert st.packed_encoder
    _run_mix(E, st, env, lens)
    assert st.counter("enc_rows") == sum(lens)
    assert st.fetch("enc", B).shape == (B, env, MICRO.n_audio_state)      # the envelope's layout on the way out
    on = {w: _valid(st, w, lens) for w in WHATS + ("stem",)}
    on_walk = _walk(ctx, st, B)
    ref_rows, ref_walk = unpacked[dt, env]
    for w in WHATS:
        for b in range(B):
            assert _rows_equal(on[w][b], off[w][b]), (w, b, lens[b])
            assert _rows_equal(on[w][b], ref_rows[w][b]), (w, b, lens[b])
    for b in range(B):
        assert _rows_equal(on["stem"][b], ref_rows["stem"][b]), b         # the conv stem and its tap stay as they are
        assert _same_walk(on_walk[b], off_walk[b]) and _same_walk(on_walk[b], ref_walk[b]), b
    st.close()
    for b, n in enumerate(lens):                                 # one window alone at set_audio_ctx(n_ctx[b])
        lone = E.State(ctx, 1)
        lone.set_audio_ctx(n)
        lone.mel(PCM[b:b + 1], NS[b:b + 1], E.OHW_MEL_ZERO_TAIL, want=False)
        lone.encode(1)
        for w in WHATS:
            a = lone.fetch(w, 1)[0]
            assert a.shape[0] == n and _rows_equal(a, on[w][b]), (w, b, n)
        lone.close()


# 2. no window writes into a neighbour's rows, and every row a window owns is written
@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("env", [256, 1500])
def test_neighbours_are_not_clobbered(E, ctxs, unpacked, dt, env):
    ctx, lens = ctxs[dt], MIXES[env]
    B = len(lens)
    st = E.State(ctx, B)
    st.set_packed_encoder(True)
    other = lens[::-1]                                           # a prior packed encode under other lengths: other window starts
    st.set_audio_ctx(env)
    st.set_window_ctx(other)
    st.mel(PCM[:B], NS[:B], E.OHW_MEL_ZERO_TAIL, want=False)
    st.encode(B)
    assert st.counter("enc_rows") == sum(lens)
    st.poison("qkv")
    st.poison("att")
    _run_mix(E, st, env, lens)
    ref_rows, ref_walk = unpacked[dt, env]
    for w in WHATS:
        for b, x in enumerate(_valid(st, w, lens)):
            assert not np.isnan(x).any(), (w, b)
            assert np.array_equal(x, ref_rows[w][b]), (w, b, lens[b])
    for b, x in enumerate(_walk(ctx, st, B)):
        assert _same_walk(x, ref_walk[b]), b
    st.close()


# 3. the row counter
def test_row_counter(E, ctxs):
    ctx, env, lens = ctxs[1], 256, MIXES[256]
    B = len(lens)
    st = E.State(ctx, B)
    _run_mix(E, st, env, lens)
    assert st.counter("enc_rows") == B * env
    st.set_packed_encoder(True)
    _run_mix(E, st, env, lens)
    assert st.counter("enc_rows") == sum(lens) == 648
    _run_mix(E, st, env, [env] * B)                              # every length at the envelope: the uniform path
    assert st.counter("enc_rows") == B * env
    st.set_packed_encoder(False)
    _run_mix(E, st, env, lens)
    assert st.counter("enc_rows") == B * env
    st.close()


# 4. slices: two packed encodes of different length lists into one decode batch
@pytest.mark.parametrize("dt", [0, 1])
def test_packed_slices_fill_one_decode_batch(E, ctxs, unpacked, dt):
    ctx, env, lens = ctxs[dt], 256, MIXES[256]
    two = E.State(ctx, 5)
    two.set_packed_encoder(True)
    two.set_audio_ctx(env)
    two.set_window_ctx(lens[:3])
    two.mel(PCM[:3], NS[:3], E.OHW_MEL_ZERO_TAIL, want=False)
    two.encode_slice(3, 0, 5)
    assert two.counter("enc_rows") == sum(lens[:3])
    two.set_window_ctx(lens[3:])
    two.mel(PCM[3:5], NS[3:5], E.OHW_MEL_ZERO_TAIL, want=False)
    two.encode_slice(2, 3, 5)
    assert two.counter("enc_rows") == sum(lens[3:])
    assert [two.window_ctx(b) for b in range(5)] == lens
    ref_rows, ref_walk = unpacked[dt, env]
    for w in ("xk0", "xv1"):
        for b, x in enumerate(_valid(two, w, lens)):
            assert _rows_equal(x, ref_rows[w][b]), (w, b)
    for b, x in enumerate(_walk(ctx, two, 5)):
        assert _same_walk(x, ref_walk[b]), b
    two.close()


# 5. without lengths the switch does nothing; the refusals of set_window_ctx hold with it on
@pytest.mark.parametrize("dt", [0, 1])
def test_no_lengths_no_effect(E, ctxs, dt):
    ctx = ctxs[dt]
    runs = []
    for on in (False, True):
        st = E.State(ctx, 3)
        st.set_packed_encoder(on)
        st.set_audio_ctx(256)
        st.mel(PCM[:3], NS[:3], E.OHW_MEL_ZERO_TAIL, want=False)
        st.encode(3)
        assert st.counter("enc_rows") == 3 * 256
        runs.append(({w: st.fetch(w, 3) for w in WHATS + ("stem",)}, _walk(ctx, st, 3)))
        st.close()
    for w in WHATS + ("stem",):
        assert np.array_equal(runs[0][0][w], runs[1][0][w]), w
    assert all(_same_walk(x, y) for x, y in zip(runs[0][1], runs[1][1]))


def test_stale_stages_are_refused_with_the_switch_on(E, ctxs):
    ctx = ctxs[1]
    lens = MIXES[256][:3]
    st = E.State(ctx, 3)
    st.set_packed_encoder(True)
    _run_mix(E, st, 256, lens)
    p = ctx.default_params()
    p.n_max = 4
    one = np.full((3, 1), ctx.tok.sot, np.int32)
    good = st.decode(one, [0, 0, 0])
    decodes = (lambda: st.decode(one, [0, 0, 0]), lambda: st.decode_active(one, [0, 0, 0], [1, 1, 1]), lambda: st.greedy(3, p),
               lambda: st.greedy_ex(3, p), lambda: st.detect_language(3))

    def refused(f):
        with pytest.raises(E.WhisperError) as ex:
            f()
        assert ex.value.code == E.OHW_E_INVALID_ARG

    st.set_window_ctx([256, 64, 129])            # the lengths changed, no encode since
    for f in decodes:
        refused(f)
    refused(lambda: st.encode(3))                # the mel image was made under other lengths
    st.set_window_ctx(None)
    for f in decodes:
        refused(f)
    refused(lambda: st.encode(3))
    st.set_window_ctx(lens)                      # the lengths of the last mel and encode again: fine
    assert np.array_equal(st.decode(one, [0, 0, 0]), good)
    st.set_window_ctx(lens[:2])                  # lengths for two windows, a mel of three
    refused(lambda: st.mel(PCM[:3], NS[:3], E.OHW_MEL_ZERO_TAIL, want=False))
    st.set_window_ctx(None)                      # a slice without lengths beside a packed slice with lengths
    st.mel(PCM[2:3], NS[2:3], E.OHW_MEL_ZERO_TAIL, want=False)
    refused(lambda: st.encode_slice(1, 2, 3))
    bad = np.asarray([8, 257, 256], np.int32)
    assert E.lib().ohw_state_set_window_ctx(st.h, E._ip(bad), 3) == E.OHW_E_INVALID_ARG
    st.close()


# 6. the engine: transcribe_batch under the auto context, packed against unpacked
def test_transcribe_batch_is_the_same_packed(E, tmp_models):
    clips = [synth.synth_audio(30 + i, int(round(s * 16000))) for i, s in enumerate([1.1, 3, 5, 12, 30, 7.3])]
    eng = E.WhisperEngine.new(tmp_models("micro"), "auto", False, True, 0, E.OHW_DTYPE_F16, 4)
    eng.set_decode_policy(temperature_inc=0.0)
    eng.set_audio_ctx("auto")
    state = E.lib().ohw_engine_state(eng.h)
    got = {}
    for on in (False, True):
        eng.set_packed_encoder(on)
        assert E.lib().ohw_state_packed_encoder(state) == int(on)
        res = eng.transcribe_batch([E.AudioBuffer(c.copy(), 16000) for c in clips])
        got[on] = [(r.text,) + tuple(eng.batch_result(i)) for i, r in enumerate(res)]
        # the last batch holds the two shortest recordings: contexts 128 and 192
        assert E.lib().ohw_dbg_counter(state, b"enc_rows") == (128 + 192 if on else 2 * 192)
    assert any(len(g[2]) > 0 for g in got[True])
    assert got[True] == got[False]                                               # text, tokens, every quality field
    eng.close()
