"""The speech plan (ohw_speech_segments_host, ohw_speech_chunks_host: csrc/vad.cpp, host code only) under AddressSanitizer and
UBSan: tests/c/vad_plan_main.cpp, a stand-alone program with its own main, is compiled together with vad.cpp with the sanitizers
on the host side and run once.  Output arrays have exactly the reported size, or less, so a write behind `cap` is reported.
No GPU, and nothing is loaded into the interpreter."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_plan_functions_are_clean_under_asan_and_ubsan(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = str(tmp_path / "vad_plan_main")
    san = ["-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fsanitize=undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           "-Xarch_host", "-fno-omit-frame-pointer", "-g"]
    cmd = [hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-x", "hip"] + san + [
        os.path.join(ROOT, "openhush_amd", "csrc", "vad.cpp"), os.path.join(ROOT, "tests", "c", "vad_plan_main.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([out], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "plan ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])
