"""tests/mel_ref.py is right, its inputs are needles, and the tolerance of tests/test_gpu_mel.py follows from them - no GPU.

  the reference against the fp32 C oracle (an independent restatement) at the project's 2e-4
  the reference against the closed form of a lone impulse at 1e-12
  every mutant of the reference moves a named builder input by at least 10 x TOL_MEL (the table is printed)
  WORST_FP32 / TOL_MEL: the float32 restatement of the kernel's arithmetic against the float64 reference over every input
"""
import numpy as np
import pytest

import mel_ref as R
from openhush_amd import synth

MELS = (80, 128)                    # nano's and micro-v3's


@pytest.fixture(scope="module")
def filters():
    return {m: synth.mel_filterbank(m) for m in MELS}


@pytest.mark.parametrize("preset", ["nano", "micro-v3"])
def test_reference_matches_the_oracle(preset):
    from oracle import oracle
    hp = synth.PRESETS[preset]
    om = oracle.Model.synth(hp.as_list(), 1234)
    filt = om.mel_filters()
    assert np.array_equal(filt, synth.mel_filterbank(hp.n_mels))
    full, short = synth.synth_audio(7), synth.synth_audio(3, 48000)
    for mode in R.MODES:
        for x in (full, short):
            d = np.abs(R.log_mel_window(x, len(x), mode, filt) - om.log_mel(x, mode)).max()
            print(f"{preset} synth_audio[{len(x)}] {R.MODE_NAMES[mode]}: reference - oracle {d:.2e}")
            assert d < 2e-4
    a = R.recording_a()
    mx, omx = R.recording_max(a.pcm, filt), om.recording_max(a.pcm)
    print(f"{preset} recording_a: maximum {mx:.6f}, oracle {omx:.6f}")
    assert abs(mx - omx) < 2e-4
    for sk in (0, 3000, 5990):
        d = np.abs(R.log_mel_seek(a.pcm, sk, mx, filt) - om.log_mel_seek(a.pcm, sk, omx)).max()
        print(f"{preset} recording_a seek {sk}: reference - oracle {d:.2e}")
        assert d < 2e-4
    om.close()


@pytest.mark.parametrize("mels", MELS)
def test_a_lone_impulse_has_a_flat_spectrum(filters, mels):
    """height a at position j of a frame: the windowed frame's power is (a hann[j])^2 in every bin, so channel c of the log-mel
    before the clamp is log10((a hann[j])^2 sum(filters[c]))"""
    filt = filters[mels].astype(np.float64)
    a, at = 0.7, 4079
    x = np.zeros(R.CHUNK, np.float32)
    x[at] = a
    a = float(x[at])
    h = R.hann()
    seen = 0
    for mode in R.MODES:
        lm = R.window_log_power(x, R.CHUNK, mode, filt)
        for t in range(R.FRAMES):
            j = at - (R.HOP * t - R.N_FFT // 2)
            want = np.log10(np.maximum((a * h[j]) ** 2 * filt.sum(axis=1), 1e-10)) if 0 <= j < R.N_FFT else np.full(mels, -10.0)
            assert np.abs(lm[:, t] - want).max() < 1e-12, (mode, t, j)
            seen += 0 <= j < R.N_FFT
    assert seen == 2 * 2                # frames 25 and 26: j = 279 and 119, both on the slope


def _window_mutant(case, mut):
    def run(f):
        return R.log_mel_window(case.pcm, case.n, case.mode, f), R.log_mel_window(case.pcm, case.n, case.mode, f, mut={mut})
    return run


def _neighbour_max(f):
    tone, noise, _ = R.loudness_triplet()
    lm = R.window_log_power(noise.pcm, noise.n, noise.mode, f)
    other = R.window_log_power(tone.pcm, tone.n, tone.mode, f).max()
    return R.normalise(lm, lm.max()), R.normalise(lm, other)


def _previous_max(f):
    loud, quiet = R.recording_c()
    stale = max(R.recording_max(loud.pcm, f), R.recording_max(quiet.pcm, f))      # the running maximum was never reset
    return R.log_mel_seek(quiet.pcm, 0, R.recording_max(quiet.pcm, f), f), R.log_mel_seek(quiet.pcm, 0, stale, f)


def _chunks(f):
    """an impulse of 0.5 in silence lifts no clamp above -10, so the windows cannot show it: the maximum ohw_recording_set returns
    does (the GPU test holds it to 1e-5)"""
    b = R.recording_b(R.CHUNK - 41)
    return np.array([R.recording_max(b.pcm, f)]), np.array([R.recording_max(b.pcm, f, mut={"chunks_no_plus1"})])


def _image_mutant(mut, t_lim):
    def run(f):
        c = R.impulses(R.REFLECT)
        m = R.log_mel_window(c.pcm, c.n, c.mode, f).astype(np.float32)
        return R.image(m, len(f), 1, t_lim), R.image(m, len(f), 1, t_lim, mut={mut})
    return run


# mutant -> (the builder input that catches it, how)
CAUGHT_BY = {
    "frame_shift": ("impulses/reflect", _window_mutant(R.impulses(R.REFLECT), "frame_shift")),
    "hann_symmetric": ("bin_tone37/reflect", _window_mutant(R.bin_tone(37), "hann_symmetric")),
    "start_reflect": ("impulses/zero_tail", _window_mutant(R.impulses(R.ZERO_TAIL), "start_reflect")),
    "end_reflect": ("impulses/reflect", _window_mutant(R.impulses(R.REFLECT), "end_reflect")),
    "mode_swapped": ("bin_tone100/zero_tail", _window_mutant(R.bin_tone(100, R.ZERO_TAIL), "mode_swapped")),
    "bin_step": ("bin_tone37/reflect", _window_mutant(R.bin_tone(37), "bin_step")),
    "read_past_n": ("ragged200/reflect", _window_mutant(R.ragged(200), "read_past_n")),
    "neighbour_max": ("loudness_triplet: the noise under the tone's maximum", _neighbour_max),
    "previous_max": ("recording_c: the quiet recording under the loud one's maximum", _previous_max),
    "chunks_no_plus1": ("recording_b479959: the returned maximum", _chunks),
    "image_shift": ("image of impulses/reflect", _image_mutant("image_shift", R.FRAMES)),
    "image_keeps_tail": ("image of impulses/reflect under t_lim 74", _image_mutant("image_keeps_tail", 74)),
}


def test_the_table_names_every_mutant():
    assert set(CAUGHT_BY) == set(R.MUTANTS)


@pytest.mark.parametrize("mut", R.MUTANTS)
def test_every_mutant_is_caught(filters, mut):
    name, run = CAUGHT_BY[mut]
    right, wrong = run(filters[80])
    d = float(np.abs(right - wrong).max())
    print(f"mutant {mut}: caught by {name}: {d:.3e} = {d / R.TOL_MEL:.0f} x TOL_MEL")
    assert d >= 10 * R.TOL_MEL


def test_second_pseudo_window_boundary(filters):
    """the library's count of pseudo-windows, (n + 200) / 160 + 1 frames in 3000s, against the frames that touch a sample: it
    covers them for every n of recording (b), and it is two from n = 479800"""
    for n in R.REC_B_N + (1, 159, 160, 161, R.REC_A_N):
        covered = -(-((n + 200) // 160 + 1) // R.FRAMES) * R.FRAMES
        assert covered >= R.recording_frames(n), n
    assert [-(-((n + 200) // 160 + 1) // R.FRAMES) for n in (479799, 479800, 479801, 479959)] == [1, 2, 2, 2]
    f = filters[80]
    b = R.recording_b(R.CHUNK - 41)
    lm = R.recording_log_power(b.pcm, f)
    assert lm.shape[1] == 3001 and lm[:, 3000].max() == lm.max()        # the loudest frame is the second pseudo-window's first


def test_tolerance_from_the_float32_restatement(filters):
    worst, where = 0.0, None
    for case in R.cases():
        for mels in MELS:
            f = filters[mels]
            for i, (ref, emu) in enumerate(zip(R.reference(case, f), R.fp32_emulation(case, f))):
                assert emu.dtype == np.float32 and ref.shape == emu.shape == (mels, R.FRAMES)
                d = float(np.abs(emu.astype(np.float64) - ref).max())
                if d > worst:
                    worst, where = d, (case.name, mels, i)
    tol = min(2e-4, 32 * worst)
    print(f"worst |fp32 restatement - float64| = {worst:.3e} at {where}; mel_ref.WORST_FP32 = {R.WORST_FP32:.3e}")
    print(f"TOL_MEL = min(2e-4, 32 * worst) = {tol:.3e}; mel_ref.TOL_MEL = {R.TOL_MEL:.3e}")
    assert R.WORST_FP32 / 2 <= worst <= R.WORST_FP32 * 2
    assert R.TOL_MEL == min(2e-4, 32 * R.WORST_FP32) <= 2e-4
