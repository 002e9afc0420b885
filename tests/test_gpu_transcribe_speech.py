"""ohw_engine_transcribe_speech: the speech of each recording is found on the device (or taken from the caller's probabilities),
cut at its pauses into chunks of at most 30 s, and the chunks of all recordings run as one transcribe_batch.  Micro model file,
f16, max_batch = 4, the timestamp / end-of-text bias of the seek-loop tests so that segments carry timestamps.

The audio is noise at -60 dBFS with amplitude-modulated four-tone bursts at -20 dBFS at known times (vad_ref.burst_audio).
The CONTRACT is exact: chunk c's tokens, quality record (its log-probability figures included), segments, token and word times
are those of transcribe_batch on samples[start:end], the times moved by start / 16000 in fp32 as the shared emit path adds it.
"""
import ctypes as C

import numpy as np
import pytest

import vad_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32 = np.float32
MAX_BATCH = 4
BURSTS = {"a": (40.0, [(2.0, 6.0), (7.0, 9.5), (15.0, 21.0), (30.0, 33.0)]),       # 1 s pause: one chunk; 5.5 s and 9 s: new chunks
          "b": (12.0, [(1.0, 3.0), (8.0, 10.5)]),
          "c": (25.0, [(1.5, 12.0), (13.0, 22.5)])}                                  # one chunk of 21 s
# every recording is more than a tenth noise alone: the detector's floor is the 10 % quantile of the band energy


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from openhush_amd import engine
    assert hasattr(engine.lib(), "ohw_engine_transcribe_speech") and hasattr(engine.lib(), "ohw_engine_speech_chunks")
    return engine


@pytest.fixture(scope="module")
def recs():
    out = {k: R.burst_audio(sec, bursts, seed=11 + i) for i, (k, (sec, bursts)) in enumerate(sorted(BURSTS.items()))}
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def oracle_tokens(E):
    from openhush_amd import synth
    ctx = E.Context.synthetic(synth.PRESETS["micro"].as_list(), 1234, 0, E.OHW_DTYPE_F16)
    t = (ctx.tok.timestamp_begin, ctx.tok.eot, ctx.hp.n_vocab)
    ctx.close()
    return t


def make_engine(E, path, oracle_tokens, beam=0, auto_packed=False, heads=None):
    tok_beg, tok_eot, n_vocab = oracle_tokens
    bias = np.zeros(n_vocab, np.float32)
    bias[tok_beg:] = 8.0
    bias[tok_eot] = 26.0
    eng = E.WhisperEngine.new(path, "en", False, True, 0, E.OHW_DTYPE_F16, MAX_BATCH)
    eng.set_decode_policy(temperature_inc=0.0)
    E.lib().ohw_state_set_logit_bias(E.lib().ohw_engine_state(eng.h), bias.ctypes.data_as(C.POINTER(C.c_float)), bias.size)
    if beam:
        eng.set_beam_size(beam)
    if auto_packed:
        eng.set_audio_ctx("auto")
        eng.set_packed_encoder(True)
    if heads:
        eng.set_word_timestamps(heads)
    return eng


def speech(E, eng, pcms, probs=None):
    res = eng.transcribe_speech([E.AudioBuffer(p.copy(), 16000) for p in pcms], probs=probs)
    out = []
    for i, r in enumerate(res):
        text, toks, _, lang = eng.batch_result(i)
        tt, words, segs = eng.batch_times(i)
        ch = eng.speech_chunks(i)
        assert text == r.text and [c["quality"] for c in ch] == eng.long_batch_quality(i)
        out.append({"text": text, "language": lang, "tokens": toks, "chunks": ch, "token_times": tt, "words": words, "segments": segs,
                    "speech": eng.speech_segments(i)})
    return out


def moved(loc, off_samples, n_samples):
    """a local time on the recording's clock, as the emit path computes it in fp32: the end of the audio is the fp32 of
    (offset + length) in double, everything else the fp32 sum of the fp32 offset and the local fp32 time"""
    off = off_samples / 16000.0
    if F32(loc) == F32(n_samples / 16000.0):
        return {float(F32(off + n_samples / 16000.0)), float(F32(F32(off) + F32(loc)))}
    return {float(F32(F32(off) + F32(loc)))}


def check_contract(E, eng, pcms, got):
    """every chunk against transcribe_batch on its slice"""
    owners = [(i, c) for i in range(len(pcms)) for c in range(len(got[i]["chunks"]))]
    slices = [pcms[i][got[i]["chunks"][c]["start"]:got[i]["chunks"][c]["end"]] for i, c in owners]
    eng.transcribe_batch([E.AudioBuffer(s.copy(), 16000) for s in slices])
    local = [(eng.batch_result(k), eng.batch_times(k)) for k in range(len(slices))]
    for i in range(len(pcms)):
        toks, quality, tts, words, segs, texts = [], [], [], [], [], []
        for k, (ri, c) in enumerate(owners):
            if ri != i:
                continue
            (text, tk, q, _), (tt, wd, sg) = local[k]
            ch = got[i]["chunks"][c]
            toks += tk
            quality.append(q)
            texts.append(text)
            tts += [(t["id"], c, t["t0"], t["t1"], ch) for t in tt]
            words += [(w["text"], w["t0"], w["t1"], ch) for w in wd]
            segs += [(s["text"], s["t0"], s["t1"], ch) for s in sg]
        g = got[i]
        assert g["tokens"] == toks and [c["quality"] for c in g["chunks"]] == quality, i
        assert "".join(g["text"].split()) == "".join("".join(texts).split()), i
        assert len(g["token_times"]) == len(tts) and len(g["words"]) == len(words) and len(g["segments"]) == len(segs), i
        for a, (tid, c, t0, t1, ch) in zip(g["token_times"], tts):
            n = ch["end"] - ch["start"]
            assert a["id"] == tid and a["window"] == c and a["t0"] in moved(t0, ch["start"], n) and a["t1"] in moved(t1, ch["start"], n), (i, a)
        for have, want in ((g["words"], words), (g["segments"], segs)):
            for a, (text, t0, t1, ch) in zip(have, want):
                n = ch["end"] - ch["start"]
                assert a["text"].strip() == text.strip() and a["t0"] in moved(t0, ch["start"], n) and a["t1"] in moved(t1, ch["start"], n), (i, a)


SETTINGS = {"greedy": {}, "beam2": {"beam": 2}, "auto_ctx_packed": {"auto_packed": True}, "word_times_one_head": {"heads": [(0, 1)]}}


@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_contract_chunk_equals_batch_on_its_slice(E, recs, oracle_tokens, tmp_models, setting):
    eng = make_engine(E, tmp_models("micro"), oracle_tokens, **SETTINGS[setting])
    pcms = [recs["a"], recs["b"], recs["c"]]
    got = speech(E, eng, pcms)
    assert [len(g["chunks"]) for g in got] == [3, 2, 1]
    assert any(g["tokens"] for g in got) and any(g["segments"] for g in got)
    if setting == "word_times_one_head":
        assert any(g["words"] for g in got) and any(g["token_times"] for g in got)
    for g, p in zip(got, pcms):
        for c in g["chunks"]:
            assert 0 <= c["start"] < c["end"] <= len(p) and c["end"] - c["start"] <= 480000
    check_contract(E, eng, pcms, got)


def test_detected_segments_are_where_the_bursts_are(E, recs, oracle_tokens, tmp_models):
    eng = make_engine(E, tmp_models("micro"), oracle_tokens)
    keys = sorted(BURSTS)
    got = speech(E, eng, [recs[k] for k in keys])
    tol = 0.030 + 0.040                                   # speech_pad_ms + 40 ms
    for k, g in zip(keys, got):
        truth = BURSTS[k][1]
        assert len(g["speech"]) == len(truth), (k, g["speech"])
        for (s, e, avg), (t0, t1) in zip(g["speech"], truth):
            assert abs(s / 16000.0 - t0) <= tol + 1e-9 and abs(e / 16000.0 - t1) <= tol + 1e-9 and avg > 0.5, (k, s, e, t0, t1)
    # chunks follow the plan: recording a's first chunk holds the two segments a 1 s pause apart
    assert [(c["first_segment"], c["n_segments"]) for c in got[0]["chunks"]] == [(0, 2), (2, 1), (3, 1)]


def test_together_equals_alone_and_supplied_probabilities(E, recs, oracle_tokens, tmp_models):
    eng = make_engine(E, tmp_models("micro"), oracle_tokens)
    pcms = [recs["a"], recs["b"], recs["c"]]
    together = speech(E, eng, pcms)
    for i, p in enumerate(pcms):
        assert speech(E, eng, [p])[0] == together[i], i
    # the caller's probabilities, 512 samples per frame (Silero's): the plan is speech_chunks_host's, whatever the audio holds
    p512 = np.full((len(pcms[1]) + 511) // 512, 0.02, F32)
    p512[int(2.0 * 16000 / 512):int(6.5 * 16000 / 512)] = 0.93
    p512[int(9.0 * 16000 / 512):] = 0.8                                   # speech to the last frame
    mixed = speech(E, eng, [pcms[1], pcms[1]], probs=[(p512, 512), None])
    segs = E.speech_segments_host(p512, 512, len(pcms[1]), E.default_vad_config())
    plan = E.speech_chunks_host(segs, p512, 512, len(pcms[1]), E.default_chunk_plan())
    assert len(plan) == 2 and mixed[0]["speech"] == segs
    assert [(c["start"], c["end"], c["first_segment"], c["n_segments"]) for c in mixed[0]["chunks"]] == plan
    assert mixed[1] == together[1]                                          # no probabilities for it: the device detector
    check_contract(E, eng, [pcms[1], pcms[1]], mixed)


def test_all_noise_gives_nothing_and_launches_no_decode(E, oracle_tokens, tmp_models):
    eng = make_engine(E, tmp_models("micro"), oracle_tokens)          # a fresh engine: its state has never encoded or decoded
    noise = R.burst_audio(12.0, [], seed=5)
    res = eng.transcribe_speech([E.AudioBuffer(noise, 16000)])
    assert res[0].text == "" and eng.speech_chunks(0) == [] and eng.speech_segments(0) == [] and eng.batch_result(0)[1] == []
    assert eng.long_batch_quality(0) == [] and eng.batch_times(0) == ([], [], [])
    st = E.lib().ohw_engine_state(eng.h)
    counters = {n: E.lib().ohw_dbg_counter(st, n.encode()) for n in ("step_captures", "step_graphs", "beam_captures", "persist_launches", "enc_rows")}
    assert counters == {n: 0 for n in counters}, counters                # no encode ran and no decode step was ever captured or launched
    # and beside a recording with speech it is still empty
    both = speech(E, eng, [noise, R.burst_audio(12.0, BURSTS["b"][1], seed=12)])
    assert both[0]["text"] == "" and both[0]["chunks"] == [] and len(both[1]["chunks"]) == 2


def test_a_35_s_burst_is_cut_at_the_planted_dip(E, oracle_tokens, tmp_models):
    eng = make_engine(E, tmp_models("micro"), oracle_tokens)
    pcm = R.burst_audio(42.0, [(3.0, 38.0)], seed=21, dips=[(20.0, 20.2)])       # 200 ms: too short to end the segment
    got = speech(E, eng, [pcm])[0]
    assert len(got["speech"]) == 1 and len(got["chunks"]) == 2, (got["speech"], got["chunks"])
    c0, c1 = got["chunks"]
    assert c0["end"] == c1["start"] and 20.0 * 16000 <= c0["end"] <= 20.2 * 16000, c0        # no pad at the cut
    assert c0["end"] - c0["start"] <= 480000 and c1["end"] - c1["start"] <= 480000
    check_contract(E, eng, [pcm], [got])
