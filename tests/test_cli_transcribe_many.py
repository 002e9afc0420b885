"""`openhush transcribe-many FILE [FILE ...]`: several recordings through the long-form batch (WhisperEngine.transcribe_long_batch),
one JSON object per line in argument order with the fields of `transcribe --format json`."""
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

from conftest import ROOT
from openhush_amd import synth


def _write_wav(path, pcm):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes(np.round(pcm * 32767).astype("<i2").tobytes())


def _run(args, **kw):
    return subprocess.run([sys.executable, "-m", "openhush_amd.cli"] + args, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT),
                          capture_output=True, text=True, timeout=300, **kw)


def test_surface_without_a_device(tmp_path):
    h = _run(["transcribe-many", "--help"])
    assert h.returncode == 0
    for opt in ("FILE", "--model-path", "--prompt", "--detect-language", "--word-timestamps", "--align-heads", "--max-batch"):
        assert opt in h.stdout, opt
    _write_wav(tmp_path / "a.wav", synth.synth_audio(5, 32000))
    m = _run(["transcribe-many", str(tmp_path / "a.wav"), str(tmp_path / "missing.wav"), "--model-path", str(tmp_path / "ggml-tiny.bin")])
    assert m.returncode != 0 and "not found" in m.stderr and "missing.wav" in m.stderr and m.stdout == ""
    w = _run(["transcribe-many", str(tmp_path / "a.wav"), "--model-path", str(tmp_path / "ggml-tiny.bin"), "--word-timestamps"])
    assert w.returncode != 0 and "--align-heads" in w.stderr
    c = _run(["transcribe-many", str(tmp_path / "a.wav"), "--model-path", str(tmp_path / "ggml-tiny.bin"), "--audio-ctx", "256"])
    assert c.returncode != 0 and "--audio-ctx" in c.stderr
    assert _run(["transcribe-many", "--model-path", "x"]).returncode != 0            # no file at all


@pytest.mark.gpu
def test_two_files_print_two_lines_that_equal_the_seek_mode_of_each(tmp_path, tmp_models):
    from openhush_amd import cli, engine as E
    pcms = [np.concatenate([synth.synth_audio(61), synth.synth_audio(62, 100000)]), synth.synth_audio(63, 160000)]   # 36.25 s, 10 s
    files = [str(tmp_path / "a.wav"), str(tmp_path / "b.wav")]
    for f, p in zip(files, pcms):
        _write_wav(f, p)
    out = _run(["transcribe-many"] + files + ["--model-path", tmp_models("micro"), "--dtype", "f16", "--max-batch", "2",
                                               "--word-timestamps", "--align-heads", "0.1,1.3", "--prompt", " w1 w2"])
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().split("\n")
    assert len(lines) == 2
    docs = [json.loads(l) for l in lines]
    eng = E.WhisperEngine.new(tmp_models("micro"), "auto", False, True, 0, E.OHW_DTYPE_F16, 2)
    eng.set_window_mode(E.OHW_WINDOW_SEEK)
    eng.set_word_timestamps([(0, 1), (1, 3)])
    eng.set_initial_prompt(" w1 w2")
    for f, p, j in zip(files, pcms, docs):
        assert set(j) == {"text", "language", "duration_ms", "audio_duration_secs", "transcription_time_ms", "real_time_factor", "model",
                          "segments", "words"}
        assert E.lib().ohw_state_set_batch_invariant(E.lib().ohw_engine_state(eng.h), 1) == 0
        r = eng.transcribe(E.AudioBuffer(cli.load_wav_file(f), 16000))
        assert (j["text"], j["language"]) == (r.text, r.language) and j["model"] == "micro-s1234"
        assert abs(j["audio_duration_secs"] - len(p) / 16000.0) < 1e-6 and j["real_time_factor"] > 0
        assert j["segments"] == [{"text": s["text"], "t0": s["t0"], "t1": s["t1"]} for s in eng.last_segments()]
        assert j["words"] == [{"text": s["text"], "t0": s["t0"], "t1": s["t1"]} for s in eng.last_words()]
    assert any(d["text"] for d in docs)
    eng.close()
