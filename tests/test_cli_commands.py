"""`--commands FILE [--command-penalty X|inf]` on `openhush transcribe` and `transcribe-many`: parsed on both, bad values and bad
files refused before any model is loaded, handed to WhisperEngine.set_commands and read back through last_commands() into the
JSON (the engine is a stub there); the sharded runners take the list; one `gpu` run through the real engine."""
import json
import math
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
def test_options_parse_and_refuse_bad_values_before_any_model_load(tmp_path, cmd):
    h = _run([cmd, "--help"])
    assert h.returncode == 0 and "--commands" in h.stdout and "--command-penalty" in h.stdout
    _write_wav(tmp_path / "a.wav", synth.synth_audio(5, 32000))
    (tmp_path / "list.txt").write_text("lights on\nlights off\n# a comment\n\n")
    (tmp_path / "empty.txt").write_text("# nothing\n\n")
    missing = str(tmp_path / "ggml-none.bin")                    # a model load would fail with another message
    base = [cmd, str(tmp_path / "a.wav"), "--model-path", missing, "--commands", str(tmp_path / "list.txt")]
    for bad in ("0", "-1", "nan", "1000.5", "-inf", "x"):
        r = _run(base + ["--command-penalty", bad])
        assert r.returncode != 0 and "--command-penalty" in r.stderr and "Model loaded" not in r.stderr and r.stdout == "", (bad, r.stderr)
    for bad_file in ("empty.txt", "none.txt"):
        r = _run([cmd, str(tmp_path / "a.wav"), "--model-path", missing, "--commands", str(tmp_path / bad_file)])
        assert r.returncode != 0 and "--commands" in r.stderr and "Model loaded" not in r.stderr and r.stdout == "", (bad_file, r.stderr)
    # good values get as far as the model
    for good in ("100", "inf", "0.5", "1000"):
        r = _run(base + ["--command-penalty", good])
        assert r.returncode != 0 and "--command-penalty" not in r.stderr and "--commands" not in r.stderr, (good, r.stderr)


class _Result:
    text, language, duration_ms, segments, words = "lights off", "en", 7, [], []


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

    def set_commands(self, phrases, penalty=100.0):
        self.calls.append(("set_commands", list(phrases), penalty))

    def last_commands(self, recording=None):
        self.calls.append(("last_commands", recording))
        return [{"window": 0, "index": 1, "list_logprob": -0.25}, {"window": 1, "index": -1, "list_logprob": -math.inf}]

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
def test_options_reach_the_engine_and_the_hits_reach_the_json(tmp_path, monkeypatch, capsys, cmd):
    from openhush_amd import cli, engine as E
    monkeypatch.setattr(E, "WhisperEngine", _Engine)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    _write_wav(tmp_path / "a.wav", synth.synth_audio(5, 32000))
    (tmp_path / "list.txt").write_text("lights on\n  lights off  \n# a comment\n")
    phrases = ["lights on", "lights off"]
    cases = ((["--commands", str(tmp_path / "list.txt")], ("set_commands", phrases, 100.0)), ([], None),
             (["--command-penalty", "5"], None),                                    # a penalty without a list sets nothing
             (["--commands", str(tmp_path / "list.txt"), "--command-penalty", "inf"], ("set_commands", phrases, math.inf)),
             (["--commands", str(tmp_path / "list.txt"), "--command-penalty", "0.5", "--beam-size", "2"], ("set_commands", phrases, 0.5)))
    for extra, want in cases:
        _Engine.made.clear()
        rc = cli.main([cmd, str(tmp_path / "a.wav"), "--model-path", "ggml-stub.bin", "--format", "json", "--max-batch", "6"] + extra)
        assert rc == 0
        eng, = _Engine.made
        assert [c for c in eng.calls if c[0] == "set_commands"] == ([want] if want else [])
        names = [c[0] for c in eng.calls]
        doc = json.loads(capsys.readouterr().out)                                   # valid JSON: -inf has become null
        if want:
            run = "transcribe" if cmd == "transcribe" else "transcribe_long_batch"
            assert names.index("set_commands") < names.index(run) < names.index("last_commands")
            assert ("last_commands", None if cmd == "transcribe" else 0) in eng.calls
            assert doc["commands"] == [{"window": 0, "index": 1, "phrase": "lights off", "list_logprob": -0.25},
                                       {"window": 1, "index": -1, "phrase": None, "list_logprob": None}]
        else:
            assert "commands" not in doc and "last_commands" not in names


def test_sharded_runners_take_the_list():
    """under torch.distributed.run every rank decodes on a State of its own: the runners set the list on it"""
    from openhush_amd import engine as E, shard

    class _State:
        made = []

        def __init__(self, ctx, max_batch):
            self.commands = None
            _State.made.append(self)

        def set_command_table(self, phrases, penalty=100.0):
            self.commands = (phrases, penalty)

        def recording_set(self, pcm):
            pass

    class _Ctx:
        def default_params(self):
            return None

        def tokenize(self, raw):
            return [len(raw)] if raw.strip() else []
    real = E.State
    E.State = _State
    try:
        shard.engine_window_runner(_Ctx(), 2, commands=(["ab", "c"], 7.0))
        shard.engine_window_runner(_Ctx(), 2)
        shard.recording_window_runner(_Ctx(), 2, np.zeros(4, np.float32), commands=([[1, 2], [3]], math.inf))
    finally:
        E.State = real
    assert [s.commands for s in _State.made] == [([[2], [3], [1], [2]], 7.0), None, ([[1, 2], [3]], math.inf)]


def test_command_tokens_gives_both_forms_the_texts_index():
    from openhush_amd import engine as E

    class _Ctx:
        def tokenize(self, raw):
            return {b"ab": [1, 2], b" ab": [3], b"c": [4], b" c": [4], b"zz": [], b" zz": [], b"q": [], b" q": [9]}[raw]
    assert E.command_tokens(_Ctx(), ["ab", "c", "q"]) == ([[1, 2], [3], [4], [9]], [0, 0, 1, 2])
    with pytest.raises(ValueError, match="text 1"):
        E.command_tokens(_Ctx(), ["ab", "zz"])
    with pytest.raises(ValueError):
        E.command_tokens(_Ctx(), ["ab", [1]])
    assert E.command_tokens(_Ctx(), [[5, 6], [7]]) == ([[5, 6], [7]], [0, 1]) and E.command_tokens(_Ctx(), None) == ([], [])


@pytest.mark.gpu
def test_commands_run_through_the_cli(tmp_path, tmp_models):
    """micro model, one 30 s window under a hard list of three phrases: the text is one of them or empty, and the JSON says which"""
    pytest.importorskip("torch")
    import command_words as W
    path = W.worded_model(tmp_models("micro"), str(tmp_path / "ggml-micro-words.bin"))
    phrases = list(W.PHRASES)
    (tmp_path / "list.txt").write_text("\n".join(phrases) + "\n")
    _write_wav(tmp_path / "a.wav", synth.synth_audio(7))
    r = _run(["transcribe", str(tmp_path / "a.wav"), "--model-path", path, "--format", "json", "--max-batch", "1", "--dtype", "f16",
              "--commands", str(tmp_path / "list.txt"), "--command-penalty", "inf"])
    assert r.returncode == 0, r.stderr
    doc = json.loads(r.stdout)
    hit, = doc["commands"]
    print(doc)
    # a hard list leaves two outcomes: the window is one listed phrase, or the decode policy dropped it (no text, no phrase)
    assert hit["window"] == 0 and hit["index"] in (-1, 0, 1, 2) and doc["text"] in phrases + [""]
    assert hit["phrase"] == (phrases[hit["index"]] if hit["index"] >= 0 else None) and doc["text"] == (hit["phrase"] or "")
    assert hit["list_logprob"] is not None and hit["list_logprob"] < 0
