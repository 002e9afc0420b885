"""ohw_engine_transcribe_long_batch: several recordings of any length in one call, each through the seek loop, one window of
every live recording per decode batch (recording slots + ohw_seek_sched).  Micro model file, f16, max_batch = 2, the
timestamp / end-of-text bias of test_seek_loop_with_timestamps_matches_oracle so that timestamps drive the seeks.

The reference is each recording through transcribe() alone in OHW_WINDOW_SEEK with batch invariance on; the statement is
exact equality: text, tokens, every field of every window's quality record, segments, word and token times, language.
What makes that meaningful is asserted on the lone runs: a seek_delta other than 3000, different window counts, more live
recordings than slots (so a slot is refilled), and - under the default policy - a window that fell back.
"""
import ctypes as C

import numpy as np
import pytest

from openhush_amd import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MAX_BATCH = 2
HEADS = [(0, 1), (1, 3)]


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from openhush_amd import engine
    assert hasattr(engine.lib(), "ohw_engine_transcribe_long_batch") and hasattr(engine.lib(), "ohw_engine_long_batch_quality")
    return engine


@pytest.fixture(scope="module")
def oracle_tokens(E):
    ctx = E.Context.synthetic(synth.PRESETS["micro"].as_list(), 1234, 0, E.OHW_DTYPE_F16)
    t = (ctx.tok.timestamp_begin, ctx.tok.eot, ctx.hp.n_vocab)
    ctx.close()
    return t


@pytest.fixture(scope="module")
def recs():
    """42.5 s with a 20 dB quieter tail (the seek-loop test's), 75 s, 31 s, 12 s, 0.75 s"""
    return [np.concatenate([synth.synth_audio(41), 0.1 * synth.synth_audio(42, 200000)]).astype(np.float32),
            np.concatenate([synth.synth_audio(43), synth.synth_audio(44), synth.synth_audio(45, 240000)]).astype(np.float32),
            np.concatenate([synth.synth_audio(46), synth.synth_audio(47, 16000)]).astype(np.float32),
            synth.synth_audio(48, 192000).astype(np.float32),
            synth.synth_audio(49, 12000).astype(np.float32)]


def _engine(E, path, oracle_tokens, language="en", temperature_inc=0.0, device_ladder=False):
    tok_beg, tok_eot, n_vocab = oracle_tokens
    bias = np.zeros(n_vocab, np.float32)              # _bias(om, 8.0, 26.0) of the seek-loop test
    bias[tok_beg:] = 8.0
    bias[tok_eot] = 26.0
    eng = E.WhisperEngine.new(path, language, False, True, 0, E.OHW_DTYPE_F16, MAX_BATCH)
    if temperature_inc is not None:
        eng.set_decode_policy(temperature_inc=temperature_inc)
    eng.set_fallback_on_device(device_ladder)
    E.lib().ohw_state_set_logit_bias(E.lib().ohw_engine_state(eng.h), bias.ctypes.data_as(C.POINTER(C.c_float)), bias.size)
    return eng


def _alone(E, eng, pcm):
    """the reference: transcribe() of one recording in the seek mode with batch invariance on"""
    state = E.lib().ohw_engine_state(eng.h)
    eng.set_window_mode(E.OHW_WINDOW_SEEK)
    assert E.lib().ohw_state_set_batch_invariant(state, 1) == 0
    r = eng.transcribe(E.AudioBuffer(pcm.copy(), 16000))
    out = {"text": r.text, "language": r.language, "tokens": eng.last_tokens(), "quality": eng.last_quality_ex(),
           "token_times": eng.last_token_times(), "words": eng.last_words(), "segments": eng.last_segments()}
    E.lib().ohw_state_set_batch_invariant(state, 0)
    eng.set_window_mode(E.OHW_WINDOW_FIXED)              # the batch call runs the seek loop whatever the mode says
    return out


def _together(E, eng, pcms, languages=None):
    res = eng.transcribe_long_batch([E.AudioBuffer(p.copy(), 16000) for p in pcms], languages=languages)
    out = []
    for i, r in enumerate(res):
        text, toks, q0, lang = eng.batch_result(i)
        q = eng.long_batch_quality(i)
        tt, words, segs = eng.batch_times(i)
        assert text == r.text and lang == r.language and (not q or q[0] == q0)
        assert (tt, words, segs) == (r.token_times, r.words, r.segments)
        out.append({"text": text, "language": lang, "tokens": toks, "quality": q, "token_times": tt, "words": words, "segments": segs})
    assert eng.last_tokens() == [] and eng.last_quality_ex() == [] and eng.last_segments() == []
    return out


def _check_lone_runs_make_it_a_test(alone, n_slots):
    counts = [len(a["quality"]) for a in alone]
    deltas = [q["seek_delta"] for a in alone for q in a["quality"]]
    print(f"\nwindows per recording {counts}, distinct seek deltas {sorted(set(deltas))}, "
          f"temperatures kept {sorted({round(q['temperature'], 1) for a in alone for q in a['quality']})}")
    assert any(d != 3000 for d in deltas)                                   # timestamps really drove a seek
    assert len({c for c in counts if c > 0}) >= 2                           # recordings end in different rounds
    assert sum(1 for c in counts if c > 0) > n_slots                        # a slot is refilled
    assert any(len(a["tokens"]) > 0 for a in alone)


def test_batch_equals_every_recording_alone(E, recs, oracle_tokens, tmp_models):
    eng = _engine(E, tmp_models("micro"), oracle_tokens)
    alone = [_alone(E, eng, p) for p in recs]
    _check_lone_runs_make_it_a_test(alone, MAX_BATCH)
    together = _together(E, eng, recs)
    for i in range(len(recs)):
        assert together[i] == alone[i], i
    # under 1 s: nothing at all
    assert together[4]["text"] == "" and together[4]["tokens"] == [] and together[4]["quality"] == [] and together[4]["segments"] == []
    # another submission order: the results follow it
    perm = [3, 0, 4, 2, 1]
    assert _together(E, eng, [recs[i] for i in perm]) == [together[i] for i in perm]
    # one recording alone through the batch call, and the seek mode set on the engine: the same again
    eng.set_window_mode(E.OHW_WINDOW_SEEK)
    assert _together(E, eng, [recs[0]]) == [together[0]]
    # ohw_engine_transcribe_batch keeps refusing the seek mode and anything over 30 s
    with pytest.raises(E.WhisperError) as ex:
        eng.transcribe_batch([E.AudioBuffer(recs[3].copy(), 16000)])
    assert ex.value.code == E.OHW_E_INVALID_ARG
    eng.set_window_mode(E.OHW_WINDOW_FIXED)
    with pytest.raises(E.WhisperError) as ex:
        eng.transcribe_batch([E.AudioBuffer(recs[0].copy(), 16000)])
    assert ex.value.code == E.OHW_E_INVALID_ARG
    eng.close()


@pytest.mark.parametrize("device_ladder", [False, True])
def test_default_policy_with_the_ladder_batch_and_alone_agree(E, recs, oracle_tokens, tmp_models, device_ladder):
    """whisper.cpp's default policy: a recording's std::mt19937(0) lives across all its windows, whatever ran beside them"""
    eng = _engine(E, tmp_models("micro"), oracle_tokens, temperature_inc=None, device_ladder=device_ladder)
    alone = [_alone(E, eng, p) for p in recs]
    _check_lone_runs_make_it_a_test(alone, MAX_BATCH)
    assert any(q["temperature"] > 0 for a in alone for q in a["quality"])   # some window fell back
    together = _together(E, eng, recs)
    for i in range(len(recs)):
        assert together[i]["tokens"] == alone[i]["tokens"], i               # token for token first: the shorter message
        assert together[i] == alone[i], i
    eng.close()


def test_word_timestamps_prompt_and_languages(E, recs, oracle_tokens, tmp_models):
    path = tmp_models("micro")
    pcms = [recs[0], (recs[2] * 1e-3).astype(np.float32), recs[3], recs[4]]
    prompt = [5, 6, 7, 8, 9, 10, 11] * 4
    # detection per recording, on its first window, kept for its later windows
    det = _engine(E, path, oracle_tokens, language="auto")
    det.set_detect_language(True)
    det.set_word_timestamps(HEADS)
    det.set_initial_prompt(prompt)
    alone = [_alone(E, det, p) for p in pcms]
    assert any(len(a["words"]) > 0 for a in alone) and any(len(a["quality"]) > 1 for a in alone)
    together = _together(E, det, pcms)
    print(f"\ndetected {[a['language'] for a in alone]}")
    for i in range(len(pcms)):
        assert together[i]["language"] == alone[i]["language"], i
        assert (together[i]["token_times"], together[i]["words"], together[i]["segments"]) == \
               (alone[i]["token_times"], alone[i]["words"], alone[i]["segments"]), i
        assert together[i] == alone[i], i
    # without the prompt the tokens differ: it really sat in front of the windows
    det.set_initial_prompt(None)
    assert [t["tokens"] for t in _together(E, det, pcms)] != [t["tokens"] for t in together]
    # a language per recording: each equals an engine created with that code; None detects that recording
    det.set_initial_prompt(prompt)
    want = ["de", 3, None, "haw"]
    got = _together(E, det, pcms, languages=want)
    for i, code in enumerate(["de", "es", None, "haw"]):
        if code is None:
            assert got[i] == alone[i], i
            continue
        one = _engine(E, path, oracle_tokens, language=code)
        one.set_word_timestamps(HEADS)
        one.set_initial_prompt(prompt)
        assert got[i] == _alone(E, one, pcms[i]), (i, code)
        one.close()
    assert len({g["language"] for g in got}) >= 3
    with pytest.raises(E.WhisperError) as ex:
        _together(E, det, pcms[:2], languages=[0, 99])
    assert ex.value.code == E.OHW_E_INVALID_ARG and "recording 1" in str(ex.value)
    det.close()


def test_a_recording_that_fails_validation_is_refused_by_index(E, recs, oracle_tokens, tmp_models):
    eng = _engine(E, tmp_models("micro"), oracle_tokens)
    bad = recs[3].copy()
    bad[100] = np.nan
    with pytest.raises(E.ValidationFailed) as ex:
        _together(E, eng, [recs[3], recs[4], bad])
    assert ex.value.code == E.OHW_E_VALIDATION and "recording 2" in str(ex.value) and "NaN" in str(ex.value)
    with pytest.raises(E.WhisperError):
        eng.batch_result(0)                                                  # the failed call left no results
    with pytest.raises(E.WhisperError):
        eng.long_batch_quality(0)
    with pytest.raises(E.ValidationFailed) as ex:
        _together(E, eng, [recs[3], np.zeros(100, np.float32)])              # too short to be audio at all
    assert "recording 1" in str(ex.value)
    assert eng.transcribe_long_batch([]) == []
    eng.close()
