"""Reduced audio context, the parts that need no GPU: the context rule (ohw_audio_ctx_for and its Python mirror) and the
oracle facts the GPU tests of tests/test_gpu_audio_ctx.py rest on - a reference model made with n_audio_ctx = C is the full
model with the first C positional rows, and its encoder reads mel frames 0 .. 2C of the 3000-frame window only (so zeroing
the frames from 2C on makes it exactly whisper.cpp's audio_ctx encoder: frame 2C is then padding).
"""
import numpy as np
import pytest

from openhush_amd import synth


@pytest.fixture(scope="module")
def E():
    from openhush_amd import engine
    engine.lib()
    return engine


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o
    return o


def _rule(n):
    pos = -(-n // 320) + 32
    return min(1500, -(-pos // 64) * 64)


def test_ctx_rule_c_and_python_agree_on_a_sweep(E):
    L = E.lib()
    ns = list(range(0, 2000)) + list(range(2000, 520000, 137)) + [319, 320, 321, 460800, 460801, 480000, 480001, 10 ** 9]
    for n in ns:
        want = _rule(n)
        assert E.audio_ctx_for(n) == want, n
        assert int(L.ohw_audio_ctx_for(n)) == want, n
    for n in ns:      # a multiple of the key block (or the model's 1500), and it covers the audio with 0.64 s to spare
        c = E.audio_ctx_for(n)
        assert c == 1500 or (c % 64 == 0 and c * 320 >= n + 32 * 320), n


def test_ctx_rule_pinned_values(E):
    L = E.lib()
    for n, want in ((17600, 128), (80000, 320), (480000, 1500)):
        assert E.audio_ctx_for(n) == want and int(L.ohw_audio_ctx_for(n)) == want, n
    # the rule as stated reaches 1500 once ceil(n / 320) + 32 exceeds 1472, i.e. past 28.8 s (28.1 s rounds to 1472)
    for n in (460801, 461000, 470000, 480000, 500000):
        assert E.audio_ctx_for(n) == 1500 and int(L.ohw_audio_ctx_for(n)) == 1500, n
    assert E.audio_ctx_for(int(28.1 * 16000)) == 1472
    assert E.audio_ctx_for(0) == 64 and int(L.ohw_audio_ctx_for(-5)) == 64


def test_audio_ctx_argument_forms(E):
    assert E._audio_ctx_arg(0) == 0 and E._audio_ctx_arg(None) == 0 and E._audio_ctx_arg("auto") == -1
    assert E._audio_ctx_arg("256") == 256 and E._audio_ctx_arg(320) == 320
    assert E._audio_ctx_arg(-1) == -1 and E._audio_ctx_arg(E._audio_ctx_arg("auto")) == -1      # the C ABI's own value passes through
    with pytest.raises(ValueError):
        E._audio_ctx_arg(-3)
    for sym in ("ohw_state_set_audio_ctx", "ohw_state_audio_ctx", "ohw_engine_set_audio_ctx", "ohw_pool_set_audio_ctx", "ohw_dbg_gemm_small"):
        assert hasattr(E.lib(), sym) and sym in E.EXPORTS


@pytest.mark.parametrize("C", [8, 63, 250, 256, 750])
def test_reduced_context_oracle_is_the_full_model_with_a_position_prefix(oracle, C):
    hp = synth.PRESETS["micro"]
    full = oracle.Model.synth(hp.as_list(), 1234)
    hl = hp.as_list()
    hl[1] = C
    red = oracle.Model.synth(hl, 1234)
    assert red.n_audio_ctx == C
    names = full.tensor_names()
    assert red.tensor_names() == names
    d = hp.n_audio_state
    for n in names:
        a, b = full.tensor(n), red.tensor(n)
        if n == "encoder.positional_embedding":
            assert b.size == C * d and np.array_equal(a[:C * d], b)       # the first C rows, bit for bit
        else:
            assert np.array_equal(a, b), n
    # encode reads frames 0 .. 2C only: with the frames from 2C on zeroed, what they held before does not matter
    rng = np.random.default_rng(C)
    mel_a = rng.standard_normal((hp.n_mels, 3000)).astype(np.float32) * 0.3
    mel_b = mel_a.copy()
    mel_b[:, 2 * C:] = rng.standard_normal((hp.n_mels, 3000 - 2 * C)).astype(np.float32)
    za, zb = mel_a.copy(), mel_b.copy()
    za[:, 2 * C:] = 0
    zb[:, 2 * C:] = 0
    ea, eb = red.encode(za), red.encode(zb)
    assert ea.shape == (C, d) and np.array_equal(ea, eb)
    # and the zeroing is not idle: frame 2C is conv1's right padding, so unzeroed audio there changes the last position
    assert not np.array_equal(red.encode(mel_b)[-1], eb[-1])
    full.close()
    red.close()
