"""`--beam-size K` on `openhush transcribe` and `transcribe-many`: parsed on both, 1 and 6 refused before any model is loaded, and
handed to WhisperEngine.set_beam_size.  No GPU: the engine is a stub."""
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


def _run(args):
    return subprocess.run([sys.executable, "-m", "openhush_amd.cli"] + args, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT),
                          capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("cmd", ["transcribe", "transcribe-many"])
def test_option_parses_and_refuses_bad_sizes_before_any_model_load(tmp_path, cmd):
    h = _run([cmd, "--help"])
    assert h.returncode == 0 and "--beam-size" in h.stdout
    _write_wav(tmp_path / "a.wav", synth.synth_audio(5, 32000))
    missing = str(tmp_path / "ggml-none.bin")                    # a model load would fail with another message
    for bad in ("1", "6", "-2", "x"):
        r = _run([cmd, str(tmp_path / "a.wav"), "--model-path", missing, "--beam-size", bad])
        assert r.returncode != 0 and "--beam-size" in r.stderr and "Model loaded" not in r.stderr and r.stdout == "", (bad, r.stderr)
    r = _run([cmd, str(tmp_path / "a.wav"), "--model-path", missing, "--beam-size", "5", "--max-batch", "4"])
    assert r.returncode != 0 and "--max-batch" in r.stderr and "--beam-size" in r.stderr
    # a good size gets as far as the model
    r = _run([cmd, str(tmp_path / "a.wav"), "--model-path", missing, "--beam-size", "5"])
    assert r.returncode != 0 and "--beam-size" not in r.stderr


class _Result:
    text, language, duration_ms, segments, words = "hello", "en", 7, [], []


class _Engine:
    made = []

    def __init__(self):
        self.calls = []
        _Engine.made.append(self)

    @classmethod
    def new(cls, *a):
        e = cls()
        e.calls.append(("new", a[-1]))
        return e

    def set_beam_size(self, k):
        self.calls.append(("set_beam_size", k))

    def set_initial_prompt(self, t):
        self.calls.append(("set_initial_prompt", t))

    def transcribe(self, audio):
        self.calls.append(("transcribe",))
        return _Result()

    def transcribe_long_batch(self, audios):
        self.calls.append(("transcribe_long_batch", len(audios)))
        return [_Result() for _ in audios]

    def close(self):
        pass


@pytest.mark.parametrize("cmd", ["transcribe", "transcribe-many"])
def test_option_reaches_the_engine_setter(tmp_path, monkeypatch, capsys, cmd):
    from openhush_amd import cli, engine as E
    monkeypatch.setattr(E, "WhisperEngine", _Engine)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    _write_wav(tmp_path / "a.wav", synth.synth_audio(5, 32000))
    for extra, want in ((["--beam-size", "3"], [("set_beam_size", 3)]), ([], []), (["--beam-size", "0"], [])):
        _Engine.made.clear()
        rc = cli.main([cmd, str(tmp_path / "a.wav"), "--model-path", "ggml-stub.bin", "--format", "json", "--max-batch", "6"] + extra)
        assert rc == 0
        eng, = _Engine.made
        assert [c for c in eng.calls if c[0] == "set_beam_size"] == want
        names = [c[0] for c in eng.calls]
        if want:
            assert names.index("set_beam_size") < names.index("transcribe" if cmd == "transcribe" else "transcribe_long_batch")
        assert "hello" in capsys.readouterr().out
