"""Language detection in the engine, the batch transcribe and the pool (ohw_engine_set_detect_language,
ohw_engine_transcribe_batch_lang, ohw_pool_set_detect_language).  Micro model file, f16.

The statement is always token equality with an engine created with the detected (or given) language code: the detection
only chooses the id, everything behind it is the explicit-language path.  The synthetic model does not separate
synth.synth_audio seeds by language (all detect 91), so some clips are attenuated by 60 dB: on the CPU oracle the five clips
below detect 91, 84, 84, 69 and 91 at their own contexts (margins 2.3, 0.39, 1.3, 1.2 and 5.2 logits)."""
import ctypes as C

import numpy as np
import pytest

from openhush_amd import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SECONDS = [1.1, 3, 5, 12, 30]
GAIN = [1.0, 1e-3, 1e-3, 1e-3, 1.0]
MAX_BATCH = 2


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from openhush_amd import engine
    assert hasattr(engine.lib(), "ohw_state_set_window_lang")
    assert hasattr(engine.lib(), "ohw_engine_set_detect_language")
    return engine


@pytest.fixture(scope="module")
def clips():
    return [(synth.synth_audio(30 + i, int(round(s * 16000))) * g).astype(np.float32) for i, (s, g) in enumerate(zip(SECONDS, GAIN))]


@pytest.fixture(scope="module")
def long_pcm():
    return np.concatenate([synth.synth_audio(70), synth.synth_audio(71), synth.synth_audio(72, 160000)])        # 70 s: 3 windows


def _engine(E, path, language="auto", detect=False, max_batch=MAX_BATCH, temperature_inc=0.0, audio_ctx="auto"):
    eng = E.WhisperEngine.new(path, language, False, True, 0, E.OHW_DTYPE_F16, max_batch)
    if temperature_inc is not None:
        eng.set_decode_policy(temperature_inc=temperature_inc)
    if audio_ctx is not None:
        eng.set_audio_ctx(audio_ctx)
    if detect:
        eng.set_detect_language(True)
    return eng


def _batch(E, eng, pcms, languages=None):
    """[(language, tokens, text)] per recording"""
    res = eng.transcribe_batch([E.AudioBuffer(p.copy(), 16000) for p in pcms], languages=languages) if languages is not None else \
        eng.transcribe_batch([E.AudioBuffer(p.copy(), 16000) for p in pcms])
    out = []
    for i, r in enumerate(res):
        text, toks, q, lang = eng.batch_result(i)
        assert text == r.text and lang == r.language
        out.append((lang, toks, text))
    return out


@pytest.fixture(scope="module")
def explicit(E, tmp_models):
    """tokens of one clip on an engine created with an explicit language code (cached per code and clip)"""
    engines, cache = {}, {}

    def get(code, key, pcm):
        if (code, key) not in cache:
            if code not in engines:
                engines[code] = _engine(E, tmp_models("micro"), code)
            r = _batch(E, engines[code], [pcm])[0]
            assert r[0] == code
            cache[(code, key)] = r[1]
        return cache[(code, key)]
    yield get
    for e in engines.values():
        e.close()


def test_detection_off_is_todays_behaviour(E, clips, long_pcm, tmp_models):
    path = tmp_models("micro")
    auto, en = _engine(E, path), _engine(E, path, "en")
    auto.set_detect_language(False)
    a, b = _batch(E, auto, clips), _batch(E, en, clips)
    assert a == b and all(r[0] == "en" for r in a) and any(len(r[1]) > 0 for r in a)
    ra, rb = auto.transcribe(E.AudioBuffer(long_pcm, 16000)), en.transcribe(E.AudioBuffer(long_pcm, 16000))
    assert ra.language == rb.language == "en" and ra.text == rb.text and auto.last_tokens() == en.last_tokens() and len(auto.last_tokens()) > 0
    assert auto.last_language() == (0, "en", 1.0)
    # an explicit language is unaffected by the setting
    en.set_detect_language(True)
    assert _batch(E, en, clips) == b
    auto.close()
    en.close()


def test_batch_detects_every_recording_on_its_own(E, clips, explicit, tmp_models):
    eng = _engine(E, tmp_models("micro"), detect=True)
    together = _batch(E, eng, clips)
    langs = [r[0] for r in together]
    print(f"\ndetected {langs}, tokens {[len(r[1]) for r in together]}")
    assert len(set(langs)) >= 2, langs                      # the clips were chosen to separate (module docstring)
    assert any(len(r[1]) > 0 for r in together)
    for i, c in enumerate(clips):
        assert _batch(E, eng, [c])[0] == together[i], i                          # language, tokens and text of the clip alone
        assert together[i][1] == explicit(langs[i], i, c), (i, langs[i])      # and of an engine created with that code
    perm = [3, 0, 4, 2, 1]
    assert _batch(E, eng, [clips[i] for i in perm]) == [together[i] for i in perm]
    eng.close()


def test_languages_per_recording_equal_the_per_language_engines(E, clips, explicit, tmp_models):
    eng = _engine(E, tmp_models("micro"))                   # detection off: the caller's languages alone decide
    want = ["de", 3, "haw", "en", None]
    got = _batch(E, eng, clips, languages=want)
    codes = ["de", "es", "haw", "en"]
    for i, code in enumerate(codes):
        assert got[i][0] == code and got[i][1] == explicit(code, i, clips[i]), (i, code)
    det = _engine(E, tmp_models("micro"), detect=True)
    assert got[4] == _batch(E, det, [clips[4]])[0]           # None: that recording is detected
    assert _batch(E, eng, clips) == _batch(E, eng, clips, languages=None) and all(r[0] == "en" for r in _batch(E, eng, clips))
    with pytest.raises(E.WhisperError) as ex:
        _batch(E, eng, clips[:2], languages=[0, 99])
    assert ex.value.code == E.OHW_E_INVALID_ARG and "recording 1" in str(ex.value)
    det.close()
    eng.close()


def test_long_recording_detects_on_window_0_in_every_schedule(E, long_pcm, tmp_models):
    path = tmp_models("micro")
    # window 0's detection, through the staged API
    ctx = E.Context.from_file(path, 0, E.OHW_DTYPE_F16)
    st = E.State(ctx, 1)
    w0 = long_pcm[:synth.CHUNK_SAMPLES]
    st.mel(w0[None, :], [len(w0)], E.OHW_MEL_ZERO_TAIL, want=False)
    st.encode(1)
    hid, hprob = st.detect_language(1)
    st.close()
    code = E.lang_id_to_code(int(hid[0]))
    ref = _engine(E, path, code, max_batch=1)
    ref.set_schedule(E.OHW_SCHEDULE_SEQUENTIAL)
    rr = ref.transcribe(E.AudioBuffer(long_pcm, 16000))
    want = ref.last_tokens()
    assert rr.language == code and len(want) > 0
    ref.close()
    eng = _engine(E, path, detect=True, max_batch=1)
    for sched in (E.OHW_SCHEDULE_SEQUENTIAL, E.OHW_SCHEDULE_PIPELINE, E.OHW_SCHEDULE_LANES):
        eng.set_schedule(sched)
        r = eng.transcribe(E.AudioBuffer(long_pcm, 16000))
        i, c, pr = eng.last_language()
        assert (i, c, r.language) == (int(hid[0]), code, code), sched
        assert abs(pr - float(hprob[0, i])) < 1e-5
        assert eng.last_tokens() == want and r.text == rr.text, sched
    eng.close()


def test_host_and_device_ladder_agree_in_a_mixed_language_batch(E, clips, tmp_models):
    path = tmp_models("micro")
    ctx = E.Context.synthetic(synth.PRESETS["micro"].as_list(), 1234, 0, E.OHW_DTYPE_F16)
    bias = np.zeros(ctx.hp.n_vocab, np.float32)
    bias[ctx.tok.timestamp_begin:] = 6.0
    bias[ctx.tok.eot] = 27.0
    ctx.close()
    runs = {}
    for device_ladder in (False, True):
        eng = _engine(E, path, detect=True, temperature_inc=None)           # whisper.cpp's default ladder
        eng.set_fallback_on_device(device_ladder)
        E.lib().ohw_state_set_logit_bias(E.lib().ohw_engine_state(eng.h), bias.ctypes.data_as(C.POINTER(C.c_float)), bias.size)
        together = _batch(E, eng, clips)
        temps = [eng.batch_result(i)[2]["temperature"] for i in range(len(clips))]
        print(f"\ndevice ladder {device_ladder}: languages {[r[0] for r in together]} temperatures {[round(t, 1) for t in temps]}")
        for i, c in enumerate(clips):
            assert _batch(E, eng, [c])[0] == together[i], (device_ladder, i)
        runs[device_ladder] = (together, temps)
        eng.close()
    assert runs[False][0] == runs[True][0]                   # per recording: language, tokens, text
    assert runs[False][1] == runs[True][1]
    assert len(set(r[0] for r in runs[False][0])) >= 2 and any(t > 0 for t in runs[False][1])      # mixed languages, and the ladder ran


def test_pool_listing_device_0_twice_reports_the_single_engines_result(E, long_pcm, tmp_models):
    path = tmp_models("micro")
    eng = _engine(E, path, detect=True, audio_ctx=None)
    r = eng.transcribe(E.AudioBuffer(long_pcm, 16000))
    want = (r.language, r.text, eng.last_tokens())
    eng.close()
    pool = E.EnginePool(path, "auto", False, [0, 0], E.OHW_DTYPE_F16, MAX_BATCH)
    pool.set_decode_policy(temperature_inc=0.0)
    off = pool.transcribe(E.AudioBuffer(long_pcm, 16000))
    assert off.language == "en"
    pool.set_detect_language(True)
    p = pool.transcribe(E.AudioBuffer(long_pcm, 16000))
    assert (p.language, p.text, pool.last_tokens()) == want and len(want[2]) > 0
    assert E.Pool is E.EnginePool
    pool.close()
