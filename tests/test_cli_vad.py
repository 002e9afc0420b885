"""`openhush transcribe --vad` and `transcribe-many --vad`: speech-aware windows from the command line
(WhisperEngine.transcribe_speech); the JSON gains "chunks": [{"start": s, "end": s}] in seconds."""
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

import vad_ref as R
from conftest import ROOT


def _write_wav(path, pcm):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes(np.round(pcm * 32767).astype("<i2").tobytes())


def _run(args, **kw):
    return subprocess.run([sys.executable, "-m", "openhush_amd.cli"] + args, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT),
                          capture_output=True, text=True, timeout=300, **kw)


def test_surface_without_a_device(tmp_path):
    for cmd in ("transcribe", "transcribe-many"):
        h = _run([cmd, "--help"])
        assert h.returncode == 0
        for opt in ("--vad", "--vad-threshold", "--vad-min-silence-ms", "--vad-max-gap-ms"):
            assert opt in h.stdout, (cmd, opt)
    _write_wav(tmp_path / "a.wav", R.burst_audio(3.0, [(1.0, 2.0)]))
    model = str(tmp_path / "ggml-tiny.bin")
    a = _run(["transcribe", str(tmp_path / "a.wav"), "--model-path", model, "--vad-threshold", "0.4"])
    assert a.returncode != 0 and "--vad" in a.stderr                                   # the knobs need --vad
    b = _run(["transcribe", str(tmp_path / "a.wav"), "--model-path", model, "--vad", "--vad-threshold", "1.5"])
    assert b.returncode != 0 and "--vad-threshold" in b.stderr
    c = _run(["transcribe", str(tmp_path / "a.wav"), "--model-path", model, "--vad", "--mel", "recording"])
    assert c.returncode != 0 and "--mel" in c.stderr
    d = _run(["transcribe-many", str(tmp_path / "a.wav"), "--model-path", model, "--vad", "--carry-context"])
    assert d.returncode != 0 and "--carry-context" in d.stderr


@pytest.mark.gpu
def test_vad_json_and_text(tmp_path, tmp_models):
    from openhush_amd import cli, engine as E
    pcms = [R.burst_audio(14.0, [(1.0, 4.0), (9.0, 12.0)], seed=31), R.burst_audio(12.0, [], seed=32)]     # two chunks; noise alone
    files = [str(tmp_path / "a.wav"), str(tmp_path / "b.wav")]
    for f, p in zip(files, pcms):
        _write_wav(f, p)
    model = tmp_models("micro")
    eng = E.WhisperEngine.new(model, "auto", False, True, 0, E.OHW_DTYPE_F16, 2)
    want = eng.transcribe_speech([E.AudioBuffer(cli.load_wav_file(f), 16000) for f in files])
    chunks = [[{"start": c["start"] / 16000, "end": c["end"] / 16000} for c in eng.speech_chunks(i)] for i in range(2)]
    assert len(chunks[0]) == 2 and chunks[1] == [] and want[1].text == ""
    assert abs(chunks[0][0]["start"] - 0.97) < 0.05 and abs(chunks[0][1]["end"] - 12.03) < 0.05
    # one file, JSON
    one = _run(["transcribe", files[0], "--model-path", model, "--dtype", "f16", "--max-batch", "2", "--vad", "--format", "json"])
    assert one.returncode == 0, one.stderr
    j = json.loads(one.stdout)
    assert set(j) == {"text", "language", "duration_ms", "audio_duration_secs", "transcription_time_ms", "real_time_factor", "model", "chunks"}
    assert (j["text"], j["language"], j["chunks"]) == (want[0].text, want[0].language, chunks[0])
    # one file, text, a wider gap: the two segments are one chunk, and the transcript block is that of the engine under that plan
    plan = E.default_chunk_plan()
    plan.max_gap_ms = 6000
    eng.set_vad(None, None, plan)
    wide = eng.transcribe_speech([E.AudioBuffer(cli.load_wav_file(files[0]), 16000)])[0]
    assert len(eng.speech_chunks(0)) == 1
    eng.set_vad()
    txt = _run(["transcribe", files[0], "--model-path", model, "--dtype", "f16", "--max-batch", "2", "--vad", "--vad-max-gap-ms", "6000"])
    assert txt.returncode == 0, txt.stderr
    assert "--- Transcription ---\n" + wide.text + "\n---" in txt.stdout
    # many files: one line each, the all-noise file with empty text and no chunks
    many = _run(["transcribe-many"] + files + ["--model-path", model, "--dtype", "f16", "--max-batch", "2", "--vad", "--audio-ctx", "auto"])
    assert many.returncode == 0, many.stderr
    docs = [json.loads(l) for l in many.stdout.strip().split("\n")]
    assert len(docs) == 2 and [d["chunks"] for d in docs] == chunks and docs[1]["text"] == ""
    eng.set_audio_ctx("auto")
    want_auto = eng.transcribe_speech([E.AudioBuffer(cli.load_wav_file(f), 16000) for f in files])
    assert [d["text"] for d in docs] == [r.text for r in want_auto]
    eng.close()
