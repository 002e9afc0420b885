"""`transcribe-many --carry-context [--max-context N]`: parsed, bad values refused before any model is loaded, and handed to
WhisperEngine.set_carry_context before the call.  No GPU: the engine is a stub."""
import wave

import numpy as np
import pytest

from openhush_amd import synth


def _write_wav(path, pcm):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes(np.round(pcm * 32767).astype("<i2").tobytes())


class _Result:
    text, language, duration_ms, segments, words = "hello", "en", 7, [], []


class _Engine:
    made = []

    def __init__(self):
        self.calls = []
        _Engine.made.append(self)

    @classmethod
    def new(cls, *a):
        return cls()

    def set_carry_context(self, n=-1):
        self.calls.append(("set_carry_context", n))

    def set_initial_prompt(self, t):
        self.calls.append(("set_initial_prompt", t))

    def transcribe_long_batch(self, audios):
        self.calls.append(("transcribe_long_batch", len(audios)))
        return [_Result() for _ in audios]

    def close(self):
        pass


def test_options_reach_the_engine_setter(tmp_path, monkeypatch, capsys):
    from openhush_amd import cli, engine as E
    monkeypatch.setattr(E, "WhisperEngine", _Engine)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    _write_wav(tmp_path / "a.wav", synth.synth_audio(5, 32000))
    base = ["transcribe-many", str(tmp_path / "a.wav"), "--model-path", "ggml-stub.bin"]
    for extra, want in (([], []), (["--carry-context"], [("set_carry_context", -1)]),
                        (["--carry-context", "--max-context", "64"], [("set_carry_context", 64)]),
                        (["--carry-context", "--max-context", "0"], [])):
        _Engine.made.clear()
        assert cli.main(base + extra) == 0
        eng, = _Engine.made
        assert [c for c in eng.calls if c[0] == "set_carry_context"] == want
        names = [c[0] for c in eng.calls]
        if want:
            assert names.index("set_carry_context") < names.index("transcribe_long_batch")
        out = capsys.readouterr().out
        assert "hello" in out and "context" not in out             # the contexts do not go into the JSON
    # --max-context alone, and values below -1, are refused before any engine is made
    _Engine.made.clear()
    assert cli.main(base + ["--max-context", "8"]) == 1 and not _Engine.made
    assert "--carry-context" in capsys.readouterr().err
    for bad in ("-2", "x"):
        with pytest.raises(SystemExit):
            cli.main(base + ["--carry-context", "--max-context", bad])
        assert "--max-context" in capsys.readouterr().err and not _Engine.made
    # the option belongs to transcribe-many alone
    with pytest.raises(SystemExit):
        cli.main(["transcribe", str(tmp_path / "a.wav"), "--model-path", "ggml-stub.bin", "--carry-context"])
    capsys.readouterr()
