"""`--confidence` on `openhush transcribe` and `transcribe-many`: parsed on both, handed to WhisperEngine.set_confidence and read
back into the JSON (the engine is a stub there); one `gpu` run through the real engine."""
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


SEGMENTS = [{"text": "lights", "text_off": 0, "text_len": 6, "t0": 0.0, "t1": 1.5}, {"text": " off", "text_off": 6, "text_len": 4, "t0": 1.5, "t1": 2.0}]
WORDS = [{"text": "lights", "text_off": 0, "text_len": 6, "t0": 0.1, "t1": 0.9}, {"text": " off", "text_off": 6, "text_len": 4, "t0": 1.5, "t1": 1.9}]
TOKEN_PROBS = [{"id": 7, "window": 0, "logprob_text": -0.5, "logprob_all": -0.75, "logprob_decode": -0.25, "top_id": 7, "top_logprob_text": -0.5},
               {"id": 9, "window": 0, "logprob_text": -1.5, "logprob_all": -1.75, "logprob_decode": 0.0, "top_id": 3, "top_logprob_text": -0.125}]
WORD_PROBS = [{"text": "lights", "text_off": 0, "text_len": 6, "probability": 0.625}, {"text": " off", "text_off": 6, "text_len": 4, "probability": 0.25}]
SEGMENT_INFO = [{"avg_logprob": -0.5, "no_speech_prob": 0.125, "temperature": 0.0}, {"avg_logprob": float("nan"), "no_speech_prob": 0.125, "temperature": 0.0}]


class _Result:
    text, language, duration_ms = "lights off", "en", 7
    segments, words, token_probs, word_probs, segment_info = SEGMENTS, WORDS, TOKEN_PROBS, WORD_PROBS, SEGMENT_INFO


class _Engine:
    made = []

    def __init__(self):
        self.calls = []
        _Engine.made.append(self)

    @classmethod
    def new(cls, *a):
        return cls()

    def set_confidence(self, on=True):
        self.calls.append(("set_confidence", on))

    def set_word_timestamps(self, heads):
        self.calls.append(("set_word_timestamps", list(heads)))

    def transcribe(self, audio):
        self.calls.append(("transcribe",))
        return _Result()

    def transcribe_long_batch(self, audios):
        self.calls.append(("transcribe_long_batch", len(audios)))
        return [_Result() for _ in audios]

    last_segments = lambda self: SEGMENTS
    last_words = lambda self: WORDS
    last_token_probs = lambda self: TOKEN_PROBS
    last_word_probs = lambda self: WORD_PROBS
    last_segment_info = lambda self: SEGMENT_INFO

    def close(self):
        pass


@pytest.mark.parametrize("cmd", ["transcribe", "transcribe-many"])
def test_the_option_reaches_the_engine_and_the_records_reach_the_json(tmp_path, monkeypatch, capsys, cmd):
    from openhush_amd import cli, engine as E
    assert "--confidence" in _run([cmd, "--help"]).stdout
    monkeypatch.setattr(E, "WhisperEngine", _Engine)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    _write_wav(tmp_path / "a.wav", synth.synth_audio(5, 32000))
    base = [cmd, str(tmp_path / "a.wav"), "--model-path", "ggml-stub.bin", "--format", "json"]
    for extra in ([], ["--confidence"], ["--confidence", "--word-timestamps", "--align-heads", "0.1,1.3"]):
        _Engine.made.clear()
        assert cli.main(base + extra) == 0
        eng, = _Engine.made
        doc = json.loads(capsys.readouterr().out)                                   # valid JSON: the NaN has become null
        names = [c[0] for c in eng.calls]
        if not extra:
            assert "set_confidence" not in names and not {"tokens_conf", "word_probs"} & set(doc)
            continue
        run = "transcribe" if cmd == "transcribe" else "transcribe_long_batch"
        assert ("set_confidence", True) in eng.calls and names.index("set_confidence") < names.index(run)
        assert doc["tokens_conf"] == TOKEN_PROBS
        assert [(s["text"], s["avg_logprob"], s["no_speech_prob"]) for s in doc["segments"]] == [("lights", -0.5, 0.125), (" off", None, 0.125)]
        if "--word-timestamps" in extra:
            assert "word_probs" not in doc
            assert [(w["text"], w["t0"], w["probability"]) for w in doc["words"]] == [("lights", 0.1, 0.625), (" off", 1.5, 0.25)]
        else:
            assert "words" not in doc and doc["word_probs"] == [{"text": "lights", "probability": 0.625}, {"text": " off", "probability": 0.25}]


@pytest.mark.gpu
def test_confidence_runs_through_the_cli(tmp_path, tmp_models):
    pytest.importorskip("torch")
    path = tmp_models("micro")
    _write_wav(tmp_path / "a.wav", synth.synth_audio(7, 16000 * 12))
    plain = _run(["transcribe", str(tmp_path / "a.wav"), "--model-path", path, "--format", "json", "--max-batch", "1", "--dtype", "f16"])
    r = _run(["transcribe", str(tmp_path / "a.wav"), "--model-path", path, "--format", "json", "--max-batch", "1", "--dtype", "f16", "--confidence"])
    assert plain.returncode == 0 and r.returncode == 0, r.stderr
    doc, base = json.loads(r.stdout), json.loads(plain.stdout)
    assert doc["text"] == base["text"] and "tokens_conf" not in base
    assert len(doc["tokens_conf"]) > 0 and set(doc["tokens_conf"][0]) == {"id", "window", "logprob_text", "logprob_all", "logprob_decode", "top_id", "top_logprob_text"}
    assert all(t["logprob_all"] <= t["logprob_text"] + 1e-6 <= 1e-6 for t in doc["tokens_conf"])
    assert "".join(w["text"] for w in doc["word_probs"]).strip() == doc["text"] and all(0.0 <= w["probability"] <= 1.0 for w in doc["word_probs"])
    assert len(doc["segments"]) > 0 and all("avg_logprob" in s and 0.0 <= s["no_speech_prob"] <= 1.0 for s in doc["segments"])
