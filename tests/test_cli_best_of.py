"""`--best-of N` on `openhush transcribe` and `transcribe-many`: parsed on both, 0 and 6 refused before any model is loaded, and
handed to WhisperEngine.set_best_of (the engine is a stub there); one `gpu` run through the real engine."""
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


def _run(args):
    return subprocess.run([sys.executable, "-m", "openhush_amd.cli"] + args, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT),
                          capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("cmd", ["transcribe", "transcribe-many"])
def test_option_parses_and_refuses_bad_counts_before_any_model_load(tmp_path, cmd):
    h = _run([cmd, "--help"])
    assert h.returncode == 0 and "--best-of" in h.stdout
    _write_wav(tmp_path / "a.wav", synth.synth_audio(5, 32000))
    missing = str(tmp_path / "ggml-none.bin")                    # a model load would fail with another message
    for bad in ("0", "6", "-2", "x"):
        r = _run([cmd, str(tmp_path / "a.wav"), "--model-path", missing, "--best-of", bad])
        assert r.returncode != 0 and "--best-of" in r.stderr and "Model loaded" not in r.stderr and r.stdout == "", (bad, r.stderr)
    r = _run([cmd, str(tmp_path / "a.wav"), "--model-path", missing, "--best-of", "5", "--max-batch", "4"])
    assert r.returncode != 0 and "--max-batch" in r.stderr and "--best-of" in r.stderr
    # a good count gets as far as the model
    r = _run([cmd, str(tmp_path / "a.wav"), "--model-path", missing, "--best-of", "5"])
    assert r.returncode != 0 and "--best-of" not in r.stderr


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

    def set_best_of(self, n):
        self.calls.append(("set_best_of", n))

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
    cases = ((["--best-of", "3"], [("set_best_of", 3)]), ([], []), (["--best-of", "1"], []),
             (["--best-of", "5", "--beam-size", "2"], [("set_beam_size", 2), ("set_best_of", 5)]))
    for extra, want in cases:
        _Engine.made.clear()
        rc = cli.main([cmd, str(tmp_path / "a.wav"), "--model-path", "ggml-stub.bin", "--format", "json", "--max-batch", "6"] + extra)
        assert rc == 0
        eng, = _Engine.made
        assert [c for c in eng.calls if c[0] in ("set_best_of", "set_beam_size")] == want
        names = [c[0] for c in eng.calls]
        if want:
            assert names.index("set_best_of") < names.index("transcribe" if cmd == "transcribe" else "transcribe_long_batch")
        assert "hello" in capsys.readouterr().out


@pytest.mark.gpu
def test_best_of_run_through_the_cli(tmp_path, tmp_models):
    """micro model, one 30 s window whose T = 0 pass fails (unbiased procedural weights repeat a token), --best-of 3: the run ends
    well, prints the JSON document, and a second run gives the same text (the candidates' generators are seeded per call)."""
    pytest.importorskip("torch")
    path = tmp_models("micro")
    _write_wav(tmp_path / "a.wav", synth.synth_audio(7))
    docs = []
    for _ in range(2):
        r = _run(["transcribe", str(tmp_path / "a.wav"), "--model-path", path, "--format", "json", "--max-batch", "3", "--best-of", "3", "--dtype", "f16"])
        assert r.returncode == 0, r.stderr
        docs.append(json.loads(r.stdout))
    assert docs[0]["text"] == docs[1]["text"] and "duration_ms" in docs[0]
