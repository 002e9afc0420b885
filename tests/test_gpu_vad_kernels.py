"""The device speech detector (csrc/vad.hip: vad_band_kernel, vad_floor_kernel, vad_prob_kernel; ohw_state_vad_frames and the
ohw_dbg_vad_* entries) against tests/vad_ref.py: the band energy against float64 at a bound derived from fp32 accumulation of a
400-term DFT (vad_ref.energy_tolerance), the floor against the float32 replica EXACTLY, the probability at a bound stated from
the device expf's error (vad_ref.prob_tolerance).  Every bound is computed on the reference side; the worst observed error is
printed next to it.

Recording sizes: 250 (two frames, both cut by the end), 4801 (n % 160 = 1, 31 frames = 3 workgroups of 8 + 7) and 2.005 s
(32080 samples: n % 160 = 80, 201 frames = 25 workgroups + 1).  Inputs: an impulse at sample 0 (the reflection seam), an impulse
at n - 1 (where the zero tail starts), tones exactly on bins 7, 8, 85 and 86 (the band's edges), noise; all on a device buffer
with full-scale audio planted behind n.  Largest errors measured on an MI355X are recorded in DESIGN.md section 6."""
import numpy as np
import pytest

import vad_ref as R
from openhush_amd import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F32 = np.float32
SIZES = (250, 4801, 32080)
POISON = 1200                       # samples of full-scale audio behind n: more than a frame and its hop
GUARD = 16


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from openhush_amd import engine
    assert hasattr(engine.lib(), "ohw_state_vad_frames") and hasattr(engine.lib(), "ohw_dbg_vad_floor")
    return engine


@pytest.fixture(scope="module")
def state(E):
    ctx = E.Context.synthetic(synth.PRESETS["nano"].as_list(), 1234, 0, E.OHW_DTYPE_BF16)
    st = E.State(ctx, 1)
    yield st
    st.close()
    ctx.close()


def inputs(n):
    j = np.arange(n, dtype=np.float64)
    d = {"impulse_at_0": np.zeros(n), "impulse_at_end": np.zeros(n)}
    d["impulse_at_0"][0] = 0.5
    d["impulse_at_end"][n - 1] = 0.5
    for k in (7, 8, 85, 86):
        d[f"tone_bin_{k}"] = 0.5 * np.sin(2.0 * np.pi * k * j / 400.0 + 0.1)
    d["noise"] = np.random.default_rng(n).standard_normal(n) * 0.05
    return {k: v.astype(F32) for k, v in d.items()}


def on_device(pcm):
    """pcm followed by full-scale poison, resident in HBM -> (tensor to keep alive, address)"""
    rng = np.random.default_rng(99)
    buf = np.concatenate([pcm, np.sign(rng.standard_normal(POISON)).astype(F32)])
    t = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    return t, t.data_ptr()


def test_band_edges_are_needles_on_the_reference_side():
    """interior frames: a tone on bin 8 or 85 lies in the band, one on bin 7 or 86 only leaks into it through the Hann window's
    first sidelobe: the band energies differ by 7 dB, four orders of magnitude above the tolerance"""
    x = inputs(32080)
    e = {k: R.band_energy(x[f"tone_bin_{k}"], 32080)[5:190] for k in (7, 8, 85, 86)}
    tol = max(R.energy_tolerance(x[f"tone_bin_{k}"], 32080)[5:190].max() for k in (7, 8, 85, 86))
    assert (e[8] - e[7]).min() > 6.9 and (e[85] - e[86]).min() > 6.9 and tol < 1e-2


@pytest.mark.parametrize("n", SIZES)
def test_band_energy_against_float64(E, state, n):
    worst, worst_ratio = 0.0, 0.0
    for name, pcm in inputs(n).items():
        ref = R.band_energy(pcm, n)
        tol = R.energy_tolerance(pcm, n)
        keep, ptr = on_device(pcm)
        got = state.dbg_vad_energy(ptr, n, guard=GUARD)
        nf = R.n_frames_of(n)
        assert got.shape == (nf + GUARD,) and (got[nf:] == F32(E.OHW_DBG_SENTINEL_F32)).all(), name      # nothing behind the last frame
        err = np.abs(got[:nf].astype(np.float64) - ref)
        worst, worst_ratio = max(worst, float(err.max())), max(worst_ratio, float((err / tol).max()))
        print(f"\nvad energy n={n} {name}: max |e - float64| = {err.max():.3e} dB, bound there {tol[int(np.argmax(err / tol))]:.3e} dB")
        assert (err <= tol).all(), (name, float(err.max()))
        host = state.dbg_vad_energy(pcm, guard=GUARD)                                                    # the staged host path: same bits
        assert host.tobytes() == got.tobytes(), name
        del keep
    print(f"\nvad energy n={n}: worst error {worst:.3e} dB, worst error / bound {worst_ratio:.3f}")


def floor_cases():
    rng = np.random.default_rng(5)
    d = {"one_bin": (np.full(100, -37.3, F32), 0.10),
         "outside_the_range": (np.array([-150.0, -100.2, -100.0, 75.0, 61.0, 59.9, -99.6, 158.0, -158.0, 60.0], F32), 0.5),
         "outside_the_range_top": (np.array([-150.0, 75.0, 61.0, 158.0, 60.0, 59.6], F32), 1.0),
         # 50 frames, q = 0.1: the target is 5.  Five values in the bin of -80.25 reach it ...
         "count_lands_on_the_target": (np.concatenate([np.full(5, -80.25, F32), np.full(45, -40.0, F32)]), 0.10),
         # ... four do not, and the floor is the next occupied bin
         "count_one_short_of_the_target": (np.concatenate([np.full(4, -80.25, F32), np.full(46, -40.0, F32)]), 0.10),
         "one_frame": (np.array([-12.26], F32), 0.10),
         "two_frames": (np.array([-60.0, -20.0], F32), 0.10),
         "three_frames": (np.array([-60.0, -20.0, -30.0], F32), 0.7),
         "four_frames": (np.array([-60.0, -20.0, -30.0, -61.0], F32), 1.0),
         "several_workgroups": ((rng.standard_normal(5000) * 15.0 - 45.0).astype(F32), 0.10),
         "bin_edges": ((np.arange(-205, 125, dtype=np.float64) * 0.5).astype(F32), 0.33)}
    return d


FLOOR_CASES = floor_cases()


@pytest.mark.parametrize("name", sorted(FLOOR_CASES))
def test_floor_exact_and_probability_within_the_expf_bound(E, state, name):
    e, q = FLOOR_CASES[name]
    det = E.VadDetector(q, 9.0, 3.0)
    p, fl = state.dbg_vad_floor(e, det, guard=GUARD)
    assert fl == R.floor32(e, q), name                                                    # exactly the float32 replica
    assert (p[len(e):] == F32(E.OHW_DBG_SENTINEL_F32)).all()
    ref, z = R.probs64(e.astype(np.float64), fl, 9.0, 3.0)
    tol = R.prob_tolerance(z, 3.0)
    err = np.abs(p[:len(e)].astype(np.float64) - ref)
    print(f"\nvad prob {name}: max |p - float64| = {err.max():.3e}, bound there {tol[int(np.argmax(err / tol))]:.3e}")
    assert (err <= tol).all(), (name, float(err.max()))                                  # t < 2 and t > n - 3 included
    assert np.isfinite(p[:len(e)]).all() and (p[:len(e)] >= 0).all() and (p[:len(e)] <= 1).all()


def test_detector_refuses_bad_parameters(E, state):
    e = np.zeros(10, F32)
    for bad in ((0.0, 9.0, 3.0), (1.5, 9.0, 3.0), (0.1, 9.0, 0.0), (float("nan"), 9.0, 3.0), (0.1, float("inf"), 3.0), (0.1, 9.0, -1.0)):
        with pytest.raises(E.WhisperError) as ei:
            state.dbg_vad_floor(e, E.VadDetector(*bad))
        assert ei.value.code == E.OHW_E_INVALID_ARG
        with pytest.raises(E.WhisperError):
            state.vad_frames(np.zeros(1000, F32), detector=E.VadDetector(*bad))


def test_whole_detector_order_and_repeat(E, state):
    """vad_frames = the three kernels in a row; a second call with a shorter, quieter recording does not see the first call's
    frames (neither in the histogram nor in the smoothing); host and device samples give the same bits"""
    loud = R.burst_audio(2.005, [(0.3, 1.7)], seed=3)
    quiet = (R.burst_audio(0.31, [(0.1, 0.2)], seed=4) * 0.1)[:4801]
    p_loud, fl_loud = state.vad_frames(loud)
    p_quiet, fl_quiet = state.vad_frames(quiet)
    assert len(p_loud) == 201 and len(p_quiet) == 31
    for pcm, p, fl in ((loud, p_loud, fl_loud), (quiet, p_quiet, fl_quiet)):
        e = state.dbg_vad_energy(pcm, guard=0)
        assert fl == R.floor32(e, 0.10)
        p2, fl2 = state.dbg_vad_floor(e, guard=0)
        assert fl2 == fl and p2.tobytes() == p.tobytes()
        ref, z = R.probs64(e.astype(np.float64), fl, 9.0, 3.0)
        assert (np.abs(p.astype(np.float64) - ref) <= R.prob_tolerance(z, 3.0)).all()
    assert fl_quiet < fl_loud - 10.0                      # the quiet recording's floor is its own
    keep, ptr = on_device(quiet)
    p_dev, fl_dev = state.vad_frames(ptr, len(quiet))
    assert p_dev.tobytes() == p_quiet.tobytes() and fl_dev == fl_quiet
    del keep
    p_again, _ = state.vad_frames(loud)
    assert p_again.tobytes() == p_loud.tobytes()
    # the segments of the loud recording are where the burst is (unpadded edges within 30 ms)
    raw = R.raw_segments(p_loud, 160, R.config(min_silence_ms=200))
    assert len(raw) == 1 and abs(raw[0][0] - 30) <= 3 and abs(raw[0][1] - 170) <= 3, raw
