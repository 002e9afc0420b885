"""`--repetition-penalty X` and `--no-repeat-ngram-size N` on `openhush transcribe` and `transcribe-many`: parsed on both,
refused out of range before any model is loaded, and handed to WhisperEngine.set_repetition (the engine is a stub there); under
torch.distributed.run they reach the sharded runners; one `gpu` run through the real engine."""
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
def test_options_parse_and_refuse_values_out_of_range_before_any_model_load(tmp_path, cmd):
    h = _run([cmd, "--help"])
    assert h.returncode == 0 and "--repetition-penalty" in h.stdout and "--no-repeat-ngram-size" in h.stdout
    _write_wav(tmp_path / "a.wav", synth.synth_audio(5, 32000))
    missing = str(tmp_path / "ggml-none.bin")                    # a model load would fail with another message
    for flag, bads in (("--repetition-penalty", ("0", "0.001", "100.5", "-1.3", "nan", "x")), ("--no-repeat-ngram-size", ("-1", "33", "2.5", "x"))):
        for bad in bads:
            r = _run([cmd, str(tmp_path / "a.wav"), "--model-path", missing, flag, bad])
            assert r.returncode != 0 and flag in r.stderr and "Model loaded" not in r.stderr and r.stdout == "", (flag, bad, r.stderr)
    # good values get as far as the model
    r = _run([cmd, str(tmp_path / "a.wav"), "--model-path", missing, "--repetition-penalty", "1.3", "--no-repeat-ngram-size", "3"])
    assert r.returncode != 0 and "--repetition-penalty" not in r.stderr and "--no-repeat-ngram-size" not in r.stderr


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

    def set_repetition(self, penalty=1.0, no_repeat_ngram_size=0):
        self.calls.append(("set_repetition", penalty, no_repeat_ngram_size))

    def set_beam_size(self, k):
        self.calls.append(("set_beam_size", k))

    def transcribe(self, audio):
        self.calls.append(("transcribe",))
        return _Result()

    def transcribe_long_batch(self, audios):
        self.calls.append(("transcribe_long_batch", len(audios)))
        return [_Result() for _ in audios]

    def close(self):
        pass


@pytest.mark.parametrize("cmd", ["transcribe", "transcribe-many"])
def test_options_reach_the_engine_setter(tmp_path, monkeypatch, capsys, cmd):
    from openhush_amd import cli, engine as E
    monkeypatch.setattr(E, "WhisperEngine", _Engine)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    _write_wav(tmp_path / "a.wav", synth.synth_audio(5, 32000))
    cases = ((["--repetition-penalty", "1.3", "--no-repeat-ngram-size", "3"], [("set_repetition", 1.3, 3)]), ([], []),
             (["--repetition-penalty", "1.0", "--no-repeat-ngram-size", "0"], []),
             (["--no-repeat-ngram-size", "32"], [("set_repetition", 1.0, 32)]), (["--repetition-penalty", "0.01"], [("set_repetition", 0.01, 0)]),
             (["--repetition-penalty", "100", "--beam-size", "2"], [("set_repetition", 100.0, 0)]))
    for extra, want in cases:
        _Engine.made.clear()
        rc = cli.main([cmd, str(tmp_path / "a.wav"), "--model-path", "ggml-stub.bin", "--format", "json", "--max-batch", "6"] + extra)
        assert rc == 0
        eng, = _Engine.made
        assert [c for c in eng.calls if c[0] == "set_repetition"] == want
        names = [c[0] for c in eng.calls]
        if want:
            assert names.index("set_repetition") < names.index("transcribe" if cmd == "transcribe" else "transcribe_long_batch")
        assert "hello" in capsys.readouterr().out


def test_sharded_runners_take_the_rule():
    """under torch.distributed.run every rank decodes on a State of its own: the runners set the rule on it"""
    from openhush_amd import engine as E, shard

    class _State:
        made = []

        def __init__(self, ctx, max_batch):
            self.rule = None
            _State.made.append(self)

        def set_repeat_rule(self, penalty=1.0, ngram=0):
            self.rule = (penalty, ngram)

        def recording_set(self, pcm):
            pass

    class _Ctx:
        def default_params(self):
            return None
    real = E.State
    E.State = _State
    try:
        shard.engine_window_runner(_Ctx(), 2, repetition=(1.3, 3))
        shard.engine_window_runner(_Ctx(), 2)
        shard.recording_window_runner(_Ctx(), 2, np.zeros(4, np.float32), repetition=(1.0, 2))
    finally:
        E.State = real
    assert [s.rule for s in _State.made] == [(1.3, 3), None, (1.0, 2)]


@pytest.mark.gpu
def test_repetition_run_through_the_cli(tmp_path, tmp_models):
    """micro model, one 30 s window: the plain run repeats one token, the run under --no-repeat-ngram-size 3 prints another text"""
    pytest.importorskip("torch")
    path = tmp_models("micro")
    _write_wav(tmp_path / "a.wav", synth.synth_audio(7))
    texts = []
    for extra in ([], ["--repetition-penalty", "1.3", "--no-repeat-ngram-size", "3"]):
        r = _run(["transcribe", str(tmp_path / "a.wav"), "--model-path", path, "--format", "json", "--max-batch", "1", "--dtype", "f16"] + extra)
        assert r.returncode == 0, r.stderr
        texts.append(json.loads(r.stdout)["text"])
    assert texts[0] != texts[1]
