"""`--stitch [--stitch-overlap S]` on `openhush transcribe`: a bad overlap is refused before any model is loaded, the option
reaches WhisperEngine.set_stitch and the seams reach the JSON (the engine is a stub there), the run without it is unchanged; one
`gpu` run through the real engine."""
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


def test_a_bad_overlap_is_refused_before_any_model_load(tmp_path):
    h = _run(["transcribe", "--help"])
    assert h.returncode == 0 and "--stitch" in h.stdout and "--stitch-overlap" in h.stdout
    _write_wav(tmp_path / "a.wav", synth.synth_audio(5, 32000))
    missing = str(tmp_path / "ggml-none.bin")                    # a model load would fail with another message
    base = ["transcribe", str(tmp_path / "a.wav"), "--model-path", missing]
    for bad in ("0", "0.5", "15.02", "16", "-5", "5.01", "nan", "inf", "x"):
        r = _run(base + ["--stitch", "--stitch-overlap", bad])
        assert r.returncode != 0 and "--stitch-overlap" in r.stderr and "Model loaded" not in r.stderr and r.stdout == "", (bad, r.stderr)
    r = _run(base + ["--stitch-overlap", "5"])                   # an overlap with nothing to overlap
    assert r.returncode != 0 and "--stitch" in r.stderr and r.stdout == ""
    r = _run(["transcribe-many", str(tmp_path / "a.wav"), "--model-path", missing, "--stitch"])
    assert r.returncode != 0 and "--stitch" in r.stderr and r.stdout == ""
    for good in ([], ["--stitch-overlap", "1"], ["--stitch-overlap", "15"], ["--stitch-overlap", "2.5"], ["--stitch-overlap", "4.98"]):
        r = _run(base + ["--stitch"] + good)                     # good values get as far as the model
        assert r.returncode != 0 and "--stitch" not in r.stderr, (good, r.stderr)


class _Result:
    text, language, duration_ms, segments, words = "a b", "en", 7, [], []


class _Engine:
    made = []

    def __init__(self):
        self.calls = []
        _Engine.made.append(self)

    @classmethod
    def new(cls, *a):
        return cls()

    def set_stitch(self, overlap_s=5.0):
        self.calls.append(("set_stitch", overlap_s))

    def last_seams(self):
        self.calls.append(("last_seams",))
        return [{"left_window": 0, "shift": 6, "matches": 5, "left_cut": 40, "right_cut": 3, "n_left": 43, "n_right": 50},
                {"left_window": 1, "shift": 0, "matches": 0, "left_cut": 50, "right_cut": 0, "n_left": 50, "n_right": 9}]

    def transcribe(self, audio):
        self.calls.append(("transcribe",))
        return _Result()

    def close(self):
        pass


def test_the_option_reaches_the_engine_and_the_seams_reach_the_json(tmp_path, monkeypatch, capsys):
    from openhush_amd import cli, engine as E
    monkeypatch.setattr(E, "WhisperEngine", _Engine)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    _write_wav(tmp_path / "a.wav", synth.synth_audio(5, 62 * 16000))          # 62 s: windows at 0, 25 and 50 s under a 5 s overlap
    base = ["transcribe", str(tmp_path / "a.wav"), "--model-path", "ggml-stub.bin", "--format", "json"]
    docs = {}
    for name, extra, want in (("off", [], None), ("on", ["--stitch"], 5.0), ("on 2.5", ["--stitch", "--stitch-overlap", "2.5"], 2.5)):
        _Engine.made.clear()
        assert cli.main(base + extra) == 0
        eng, = _Engine.made
        docs[name] = json.loads(capsys.readouterr().out)
        names = [c[0] for c in eng.calls]
        if want is None:
            assert names == ["transcribe"] and "seams" not in docs[name]              # the run without --stitch is unchanged
        else:
            assert eng.calls[0] == ("set_stitch", want) and names == ["set_stitch", "transcribe", "last_seams"]
    assert docs["on"]["seams"] == [{"window": 0, "time": 27.5, "shift": 6, "matches": 5}, {"window": 1, "time": 52.5, "shift": 0, "matches": 0}]
    assert docs["on 2.5"]["seams"][1] == {"window": 1, "time": (55.0 + 57.5) / 2, "shift": 0, "matches": 0}
    drop = ("transcription_time_ms", "real_time_factor", "seams")
    assert {k: v for k, v in docs["on"].items() if k not in drop} == {k: v for k, v in docs["off"].items() if k not in drop}


@pytest.mark.gpu
def test_stitch_runs_through_the_cli(tmp_path, tmp_models):
    """micro model, 70 s: three windows and two seams under --stitch, none without; the texts are the engine's"""
    pytest.importorskip("torch")
    _write_wav(tmp_path / "a.wav", np.concatenate([synth.synth_audio(31), synth.synth_audio(32), synth.synth_audio(33)])[:70 * 16000])
    base = ["transcribe", str(tmp_path / "a.wav"), "--model-path", tmp_models("micro"), "--format", "json", "--max-batch", "4", "--dtype", "f16"]
    off, on = _run(base), _run(base + ["--stitch"])
    assert off.returncode == 0 and on.returncode == 0, (off.stderr, on.stderr)
    d_off, d_on = json.loads(off.stdout), json.loads(on.stdout)
    assert "seams" not in d_off
    assert [s["window"] for s in d_on["seams"]] == [0, 1] and [s["time"] for s in d_on["seams"]] == [27.5, 52.5]
    for s in d_on["seams"]:
        assert (s["shift"] == 0) == (s["matches"] == 0) and s["matches"] != 1
