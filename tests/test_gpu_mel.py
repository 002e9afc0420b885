"""The log-mel front end (csrc/mel.hip: mel_power_kernel, mel_normalize_kernel, and their callers in engine.hip) in every mode,
against the float64 reference of tests/mel_ref.py on its needle inputs, at mel_ref.TOL_MEL - a bound derived on the reference
side alone (tests/test_mel_ref_cpu.py), which also shows that every mistake the inputs are built for moves them by at least ten
times that.

  per window     impulses, tones on exact bins, ragged lengths with full-scale audio resident behind n (device pointer) or left
                 behind n by the previous call (host path), three loudnesses in one batch in every order
  recording      a quiet window next to a burst, the pseudo-window boundary of the maximum pass, a quiet recording after a loud
                 one on the same state, the same through the recording slots
  image          fetch("mel_t"), the only output the encoder reads: exactly the fp32 output rounded once, zero pad rows and
                 channels, zero rows behind a reduced context after a loud full-context call on the same state
  refusals       OHW_E_INVALID_ARG, and the last image is still there

The worst error against float64 of every family is printed next to the bound.  Synthetic contexts: nano (80 mels), micro-v3 (128).
"""
import functools
import itertools

import numpy as np
import pytest

import mel_ref as R
from openhush_amd import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PRESET = {80: "nano", 128: "micro-v3"}
MELS = (80, 128)
WORST = {}           # family -> worst |GPU - float64| so far
_REF = {}
_CTX = {}


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from openhush_amd import engine
    engine.lib()
    return engine


def device_guarded(fn):
    """an error that is not a refusal came from the device: nothing more is launched"""
    @functools.wraps(fn)
    def run(E, *a, **kw):
        try:
            return fn(E, *a, **kw)
        except E.WhisperError as e:
            if e.code != E.OHW_E_INVALID_ARG:
                pytest.exit(f"{fn.__name__}: the library reported {e.code} ({e}): nothing more is launched", 3)
            raise
    return run


def ctx_of(E, mels, dt=1):
    if (mels, dt) not in _CTX:
        _CTX[(mels, dt)] = E.Context.synthetic(synth.PRESETS[PRESET[mels]].as_list(), 1234, 0, dt)
    return _CTX[(mels, dt)]


@functools.lru_cache(maxsize=None)
def filters(mels):
    return synth.mel_filterbank(mels)


def ref_window(case, mels):
    """computed once per (input, mel count), shared and read-only"""
    key = (case.name, mels)
    if key not in _REF:
        _REF[key] = R.log_mel_window(case.pcm, case.n, case.mode, filters(mels))
        _REF[key].setflags(write=False)
    return _REF[key]


def ref_recording(rec, mels):
    """-> (the maximum, {seek: window})"""
    key = (rec.name, mels)
    if key not in _REF:
        mx = R.recording_max(rec.pcm, filters(mels))
        _REF[key] = (mx, {s: R.log_mel_seek(rec.pcm, s, mx, filters(mels)) for s in rec.seeks})
    return _REF[key]


def close(family, got, ref, tag):
    assert got.dtype == np.float32 and got.shape == ref.shape, tag
    d = float(np.abs(got.astype(np.float64) - ref).max())
    WORST[family] = max(WORST.get(family, 0.0), d)
    print(f"mel {family} {tag}: |GPU - float64| {d:.3e}; family so far {WORST[family]:.3e}; TOL_MEL {R.TOL_MEL:.1e}")
    assert d <= R.TOL_MEL, (tag, d, np.argwhere(np.abs(got - ref) > R.TOL_MEL)[:4].tolist())   # a NaN fails


def mel_batch(st, cases):
    """one ohw_mel of up to three windows of one mode from host memory"""
    return st.mel(np.stack([c.pcm for c in cases]), [c.n for c in cases], cases[0].mode)


@pytest.mark.parametrize("mode", R.MODES, ids=[R.MODE_NAMES[m] for m in R.MODES])
@pytest.mark.parametrize("mels", MELS)
@device_guarded
def test_impulses_and_bin_tones(E, mels, mode):
    st = E.State(ctx_of(E, mels), 3)
    cases = [R.impulses(mode)] + [R.bin_tone(k, mode) for k in R.TONE_BINS]
    for i in range(0, len(cases), 3):
        part = cases[i:i + 3]
        got = mel_batch(st, part)
        for b, c in enumerate(part):
            close("impulses" if c.name.startswith("impulses") else "bin_tone", got[b], ref_window(c, mels), f"{c.name} {mels}")
    st.close()


@pytest.mark.parametrize("mode", R.MODES, ids=[R.MODE_NAMES[m] for m in R.MODES])
@pytest.mark.parametrize("mels", MELS)
@device_guarded
def test_ragged_lengths_never_read_behind_n(E, mels, mode):
    st = E.State(ctx_of(E, mels), 1)
    loud = R.ragged(0, mode).pcm[None, :]                       # full scale everywhere
    assert np.abs(loud).max() > 0.99
    for n in R.RAGGED_N:
        c = R.ragged(n, mode)
        ref = ref_window(c, mels)
        # the poison is resident behind n
        dev = torch.from_numpy(c.pcm.copy()).to("cuda")
        st.mel_device(dev.data_ptr(), R.CHUNK, [n], mode)
        close("ragged", st.fetch("mel", 1)[0], ref, f"{c.name} {mels} device")
        # the poison is what the previous call left in the state's own copy: only n samples are uploaded
        st.mel(loud, [R.CHUNK], mode, want=False)
        got = st.mel(np.ascontiguousarray(c.pcm[None, :max(n, 1)]), [n], mode)
        close("ragged", got[0], ref, f"{c.name} {mels} host")
    st.close()


@pytest.mark.parametrize("mode", R.MODES, ids=[R.MODE_NAMES[m] for m in R.MODES])
@pytest.mark.parametrize("mels", MELS)
@device_guarded
def test_loudness_triplet_in_every_order_and_alone(E, mels, mode):
    """a positive maximum, a negative one and exact silence in one batch: every window keeps its own, whatever its neighbours"""
    st = E.State(ctx_of(E, mels), 3)
    trip = R.loudness_triplet(mode)
    first = mel_batch(st, trip)
    for b, c in enumerate(trip):
        close("triplet", first[b], ref_window(c, mels), f"{c.name} {mels}")
    assert first[0].max() > 1.0 and first[1].max() < 0.0                 # (max + 4) / 4 of a positive and of a negative maximum
    assert (first[2] == first[2][0, 0]).all() and abs(float(first[2][0, 0]) + 1.5) < 1e-6        # log10f(1e-10f) may be an ulp from -10
    for order in list(itertools.permutations(range(3)))[1:]:
        got = mel_batch(st, [trip[i] for i in order])
        for b, i in enumerate(order):
            assert np.array_equal(got[b], first[i]), (order, b)
    for i in range(3):
        assert np.array_equal(mel_batch(st, [trip[i]])[0], first[i]), i
    st.close()


@pytest.mark.parametrize("mels", MELS)
@device_guarded
def test_recording_a_quiet_window_next_to_a_burst(E, mels):
    a = R.recording_a()
    mx, wins = ref_recording(a, mels)
    st = E.State(ctx_of(E, mels), 3)
    got_mx = st.recording_set(a.pcm)
    print(f"mel recording_a {mels}: maximum {got_mx:.7f}, float64 {mx:.7f}")
    assert abs(got_mx - mx) < 1e-5
    for part in (a.seeks[:3], a.seeks[3:]):
        got = st.mel_seek(part)
        for b, sk in enumerate(part):
            close("recording_a", got[b], wins[sk], f"seek {sk} {mels}")
    tail = ((np.float32(got_mx) - np.float32(8.0)) + np.float32(4.0)) * np.float32(0.25)
    assert (st.mel_seek([a.seeks[-1]])[0] == tail).all()            # the zero tail: the clamp alone, in the kernel's fp32
    alone = R.log_mel_window(a.pcm[:R.CHUNK], R.CHUNK, R.ZERO_TAIL, filters(mels))
    assert np.abs(st.mel_seek([0])[0] - alone).max() > 0.5          # the burst of the second window clamps the first
    st.close()


@pytest.mark.parametrize("mels", MELS)
@device_guarded
def test_recording_b_the_pseudo_window_boundary(E, mels):
    """the last sample is the loudest, around the length at which the maximum pass needs a second pseudo-window"""
    st = E.State(ctx_of(E, mels), 2)
    for n in R.REC_B_N:
        b = R.recording_b(n)
        mx, wins = ref_recording(b, mels)
        got_mx = st.recording_set(b.pcm)
        print(f"mel recording_b {n} {mels}: maximum {got_mx:.7f}, float64 {mx:.7f}")
        assert abs(got_mx - mx) < 1e-5, n
        got = st.mel_seek(b.seeks)
        for i, sk in enumerate(b.seeks):
            close("recording_b", got[i], wins[sk], f"n {n} seek {sk} {mels}")
    st.close()


@pytest.mark.parametrize("mels", MELS)
@device_guarded
def test_recording_c_a_quiet_recording_after_a_loud_one(E, mels):
    loud, quiet = R.recording_c()
    st = E.State(ctx_of(E, mels), 2)
    for rec in (loud, quiet):                                      # the quiet one second: nothing of the loud one's is left
        mx, wins = ref_recording(rec, mels)
        got_mx = st.recording_set(rec.pcm)
        print(f"mel {rec.name} {mels}: maximum {got_mx:.7f}, float64 {mx:.7f}")
        assert abs(got_mx - mx) < 1e-5, rec.name
        got = st.mel_seek(rec.seeks)
        for i, sk in enumerate(rec.seeks):
            close("recording_c", got[i], wins[sk], f"{rec.name} seek {sk} {mels}")
    assert ref_recording(loud, mels)[0] > 0.0 > ref_recording(quiet, mels)[0]
    st.close()


@pytest.mark.parametrize("mels", MELS)
@device_guarded
def test_recording_a_in_a_slot_next_to_a_loud_recording(E, mels):
    a = R.recording_a()
    loud = R.Recording("recording_c_loud_x4", np.float32(4.0) * R.recording_c()[0].pcm, (0,))       # its maximum is 1.2 above recording (a)'s
    lone = E.State(ctx_of(E, mels), 3)
    lone_mx = lone.recording_set(a.pcm)
    lone_win = {s: w.copy() for s, w in zip(a.seeks[:3], lone.mel_seek(a.seeks[:3]))}
    lone.close()
    st = E.State(ctx_of(E, mels), 3)
    assert st.recording_set_slot(0, loud.pcm) > lone_mx + 1.0          # another clamp: a wrong index shows
    assert st.recording_set_slot(1, a.pcm) == lone_mx
    got = st.mel_seek_slots([1, 0, 1], [a.seeks[0], 0, a.seeks[1]])
    assert np.array_equal(got[0], lone_win[a.seeks[0]]) and np.array_equal(got[2], lone_win[a.seeks[1]])
    close("slots", got[1], ref_recording(loud, mels)[1][0], f"the loud neighbour {mels}")
    assert np.array_equal(st.mel_seek_slots([1], [a.seeks[2]])[0], lone_win[a.seeks[2]])
    st.close()


# ---- the image -------------------------------------------------------------------------------------------------------------
def check_image(st, B, mels, dt, t_lims, full, tag):
    """fetch("mel_t") is image(fetch("mel")) word for word, its pads are zero, and the fp32 output is the full-context one"""
    mel, img = st.fetch("mel", B), st.fetch("mel_t", B)
    assert img.shape == (B, R.ROWS, R.CPAD)
    for b in range(B):
        assert np.array_equal(mel[b], full[b]), (tag, b)
        assert not img[b, 0].any() and not img[b, R.ROWS - 1].any() and not img[b, :, mels:].any(), (tag, b)
        assert not img[b, 1 + t_lims[b]:].any(), (tag, b)
        want = R.image(mel[b], mels, dt, t_lims[b])
        assert np.array_equal(img[b].view(np.uint32), want.view(np.uint32)), (tag, b, np.argwhere(img[b] != want)[:4].tolist())
        if t_lims[b] > 0:
            assert img[b, 1:1 + t_lims[b], :mels].any(), (tag, b)


@pytest.mark.parametrize("dt", [0, 1], ids=["bf16", "f16"])
@pytest.mark.parametrize("mels", MELS)
@device_guarded
def test_image_is_the_fp32_output_rounded_once(E, mels, dt):
    """after ohw_mel, ohw_mel_seek and ohw_mel_seek_slots; at the full context, then under set_audio_ctx(C) and set_window_ctx, each
    time right behind a loud full-context call on the same state: rows >= 2 C hold that call's audio unless the kernel zeroes them"""
    st = E.State(ctx_of(E, mels, dt), 3)
    a, loud_rec = R.recording_a(), R.recording_c()[0]
    loud = np.stack([R.ragged(0).pcm] * 3)
    wins = [R.impulses(R.ZERO_TAIL), R.bin_tone(37, R.ZERO_TAIL), R.ragged(479999, R.ZERO_TAIL)]
    st.recording_set(a.pcm)
    st.recording_set_slot(0, loud_rec.pcm)
    st.recording_set_slot(1, a.pcm)
    paths = {"mel": lambda: mel_batch(st, wins), "mel_seek": lambda: st.mel_seek([0, 2995, 5990]),
             "mel_seek_slots": lambda: st.mel_seek_slots([1, 0, 1], [2995, 0, 0])}
    full = {}

    def loud_full_context_call():
        st.set_audio_ctx(0)
        st.mel(loud, [R.CHUNK] * 3, R.ZERO_TAIL, want=False)

    for name, run in paths.items():
        loud_full_context_call()
        full[name] = run().copy()
        check_image(st, 3, mels, dt, [R.FRAMES] * 3, full[name], f"{name} full")
    assert np.abs(st.fetch("mel_t", 3)).max() > 0.5
    for Cn in (1500, 750, 37, 1):
        for name, run in paths.items():
            loud_full_context_call()
            st.set_audio_ctx(Cn)
            run()
            check_image(st, 3, mels, dt, [2 * Cn] * 3, full[name], f"{name} audio_ctx {Cn}")
    lens = [1500, 37, 1]
    for name, run in paths.items():
        loud_full_context_call()
        st.set_window_ctx(lens)
        run()
        check_image(st, 3, mels, dt, [2 * n for n in lens], full[name], f"{name} window_ctx {lens}")
    st.set_window_ctx(None)
    st.close()


@device_guarded
def test_refusals_leave_the_last_image(E):
    st = E.State(ctx_of(E, 80), 2)
    b = R.recording_b(R.CHUNK - 41)
    st.recording_set(b.pcm)
    st.mel(R.impulses(R.REFLECT).pcm[None, :], [R.CHUNK], R.REFLECT, want=False)
    before_mel, before_img = st.fetch("mel", 1), st.fetch("mel_t", 1)
    assert before_img.any()
    x = np.zeros((1, R.CHUNK + 8), np.float32)
    n_len = (len(b.pcm) + R.CHUNK) // R.HOP
    short = np.full(R.ROWS * R.CPAD - 1, 7.0, dtype=np.float32)
    refused = [lambda: st.mel(x, [R.CHUNK + 1]),                       # n_samples above 480000
               lambda: st.mel(x[:, :1000], [1001]),                    # ... above the stride
               lambda: st.mel_seek([n_len]),                           # a seek at n_len
               lambda: E._check(E.lib().ohw_state_fetch(st.h, b"mel_t", 1, E._fp(short), short.size))]    # a short buffer
    for i, call in enumerate(refused):
        with pytest.raises(E.WhisperError) as ex:
            call()
        assert ex.value.code == E.OHW_E_INVALID_ARG, i
        assert np.array_equal(st.fetch("mel", 1), before_mel) and np.array_equal(st.fetch("mel_t", 1), before_img), i
    assert (short == 7.0).all()
    assert st.mel_seek([n_len - 1]).shape == (1, 80, R.FRAMES)        # the last frame is inside
    st.close()
