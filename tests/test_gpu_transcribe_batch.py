"""ohw_engine_transcribe_batch: several independent recordings of at most 30 s in one call, batched longest first, each at its
own audio context under the auto setting (ohw_state_set_window_ctx).  Micro model file, f16.  A recording's result must not
depend on which other recordings it was submitted with: the batch equals every recording submitted alone, exactly.
"""
import ctypes as C

import numpy as np
import pytest

from openhush_amd import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SECONDS = [1.1, 3, 5, 12, 30]
MAX_BATCH = 2


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from openhush_amd import engine
    engine.lib()
    assert hasattr(engine.lib(), "ohw_engine_transcribe_batch")
    return engine


@pytest.fixture(scope="module")
def clips():
    return [synth.synth_audio(30 + i, int(round(s * 16000))) for i, s in enumerate(SECONDS)]


def _engine(E, path, temperature_inc=0.0):
    eng = E.WhisperEngine.new(path, "auto", False, True, 0, E.OHW_DTYPE_F16, MAX_BATCH)
    if temperature_inc is not None:
        eng.set_decode_policy(temperature_inc=temperature_inc)
    return eng


def _batch(E, eng, pcms):
    res = eng.transcribe_batch([E.AudioBuffer(p.copy(), 16000) for p in pcms])
    out = []
    for i, r in enumerate(res):
        text, toks, q, lang = eng.batch_result(i)
        assert text == r.text and lang == r.language == "en"
        out.append((text, toks, q))
    return out


def test_auto_batch_equals_every_recording_alone_and_the_low_level_walk(E, clips, tmp_models):
    path = tmp_models("micro")
    eng = _engine(E, path)
    eng.set_audio_ctx("auto")
    together = _batch(E, eng, clips)
    assert len(together) == len(clips) and any(len(t[1]) > 0 for t in together)
    for i, c in enumerate(clips):
        alone = _batch(E, eng, [c])
        assert alone[0] == together[i], (i, alone[0], together[i])                 # text, tokens, every quality field
    # another submission order: the results follow it
    perm = [3, 0, 4, 2, 1]
    shuffled = _batch(E, eng, [clips[i] for i in perm])
    assert shuffled == [together[i] for i in perm]
    assert eng.last_tokens() == [] and eng.last_quality_ex() == []
    eng.close()
    # each recording's tokens are a prefix of the low-level greedy walk at ohw_audio_ctx_for(n), batch-invariant mode on
    ctx = E.Context.from_file(path, 0, E.OHW_DTYPE_F16)
    st = E.State(ctx, 1)
    st.set_batch_invariant(True)
    for i, c in enumerate(clips):
        st.set_audio_ctx(E.audio_ctx_for(len(c)))
        st.mel(c[None, :], [len(c)], E.OHW_MEL_ZERO_TAIL, want=False)
        st.encode(1)
        low = st.greedy(1)[0][0]
        toks = together[i][1]
        assert toks == low[:len(toks)], (i, toks, low)
    st.close()


def test_setting_zero_equals_transcribe_per_recording(E, clips, tmp_models):
    path = tmp_models("micro")
    eng = _engine(E, path)
    together = _batch(E, eng, clips)
    state = E.lib().ohw_engine_state(eng.h)
    for i, c in enumerate(clips):
        assert E.lib().ohw_state_set_batch_invariant(state, 1) == 0
        res = eng.transcribe(E.AudioBuffer(c.copy(), 16000))
        q = eng.last_quality_ex()
        assert len(q) == 1
        assert (res.text, eng.last_tokens(), q[0]) == together[i], i
    E.lib().ohw_state_set_batch_invariant(state, 0)
    eng.close()


def test_fixed_context_that_does_not_cover_a_recording_is_refused_by_index(E, clips, tmp_models):
    eng = _engine(E, tmp_models("micro"))
    eng.set_audio_ctx(128)
    with pytest.raises(E.WhisperError) as ex:
        _batch(E, eng, clips)
    assert ex.value.code == E.OHW_E_INVALID_ARG and "recording 1" in str(ex.value) and "128" in str(ex.value)
    assert len(_batch(E, eng, [clips[0]])) == 1                                     # 1.1 s fits 128 * 320 samples
    long = np.concatenate([clips[4], clips[0]])
    eng.set_audio_ctx(0)
    with pytest.raises(E.WhisperError) as ex:
        _batch(E, eng, [clips[0], clips[1], long])
    assert ex.value.code == E.OHW_E_INVALID_ARG and "recording 2" in str(ex.value)
    eng.set_window_mode(E.OHW_WINDOW_SEEK)
    with pytest.raises(E.WhisperError) as ex:
        _batch(E, eng, [clips[0]])
    assert ex.value.code == E.OHW_E_INVALID_ARG
    eng.close()


@pytest.mark.parametrize("device_ladder", [False, True])
def test_default_policy_with_the_ladder_on_batch_and_alone_agree(E, oracle_tokens, clips, tmp_models, device_ladder):
    """whisper.cpp's default policy (ladder 0.2 .. 1.0) with the timestamp / end-of-text bias of the ladder tests: some
    recordings fall back, each with its own std::mt19937(0)"""
    path = tmp_models("micro")
    tok_beg, tok_eot, n_vocab = oracle_tokens
    bias = np.zeros(n_vocab, np.float32)
    bias[tok_beg:] = 6.0
    bias[tok_eot] = 27.0
    eng = _engine(E, path, temperature_inc=None)
    eng.set_fallback_on_device(device_ladder)
    eng.set_audio_ctx("auto")
    E.lib().ohw_state_set_logit_bias(E.lib().ohw_engine_state(eng.h), bias.ctypes.data_as(C.POINTER(C.c_float)), bias.size)
    together = _batch(E, eng, clips)
    print(f"\ndevice ladder {device_ladder}: temperatures kept {[round(t[2]['temperature'], 1) for t in together]}, "
          f"tokens {[len(t[1]) for t in together]}")
    for i, c in enumerate(clips):
        alone = _batch(E, eng, [c])
        assert alone[0][1] == together[i][1], (i, alone[0][1], together[i][1])     # token for token
        assert alone[0] == together[i], i
    eng.close()


@pytest.fixture(scope="module")
def oracle_tokens(E):
    ctx = E.Context.synthetic(synth.PRESETS["micro"].as_list(), 1234, 0, E.OHW_DTYPE_F16)
    t = (ctx.tok.timestamp_begin, ctx.tok.eot, ctx.hp.n_vocab)
    ctx.close()
    return t


def test_a_nan_fails_validation_by_index_before_device_work(E, clips, tmp_models):
    eng = _engine(E, tmp_models("micro"))
    ok = _batch(E, eng, [clips[0]])
    bad = clips[1].copy()
    bad[100] = np.nan
    with pytest.raises(E.ValidationFailed) as ex:
        _batch(E, eng, [clips[0], clips[2], bad])
    assert ex.value.code == E.OHW_E_VALIDATION and "recording 2" in str(ex.value) and "NaN" in str(ex.value)
    with pytest.raises(E.WhisperError):
        eng.batch_result(0)                                                          # the failed call left no results
    assert _batch(E, eng, [clips[0]]) == ok
    eng.close()
