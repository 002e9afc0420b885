"""The log-mel front end (csrc/mel.hip and its callers in engine.hip) restated in float64 numpy, and the inputs the front-end
tests run: needles, on which one wrong sample, frame, bin, maximum or image row moves a value by far more than the tolerance.

The recipe (mel.hip's header): periodic Hann window of 400, hop 160, frame t covers samples 160 t - 200 .. 160 t + 199,
|rfft|^2, the model's filterbank, log10(max(., 1e-10)), a maximum, clamp to maximum - 8, (x + 4) / 4.
  per window    pos -> -pos before the start; behind sample 479999 REFLECT mirrors pos -> 2 * 479999 - pos and ZERO_TAIL reads
                zeros; samples at pos >= n are zero; the maximum is the window's own
  recording     a window at frame `seek` reads the real neighbouring samples on both sides; pos -> -pos only before the
                recording's start, zeros behind its end; the maximum is the one over every frame of the recording (the frames
                of the 30 s zero tail are log10(1e-10) = -10)
  image         [3002][128] in the 16-bit type: row 1 + t holds frame t, one conversion of the fp32 value (pack2<T>); rows 0 and
                3001, channels >= n_mels and rows of frames >= t_lim are zero

Every function takes `mut`, a set of names from MUTANTS: the same recipe with one deliberate mistake.  tests/test_mel_ref_cpu.py
shows that every mutant moves some builder input by at least ten tolerances, which is what makes the inputs needles.

fp32_window / fp32_recording repeat the recipe in float32 in the kernel's order of summation (sequential 400-term DFT with fp32
twiddles, sequential 201-term filterbank dot, log10 in fp32).  They are used for one thing only: WORST_FP32, from which the
tolerance of the GPU tests is derived - against this reference, never against the kernel.
"""
import dataclasses
import functools

import numpy as np

from openhush_amd import synth

N_FFT, HOP, N_FREQ = 400, 160, 201
CHUNK, FRAMES = 480000, 3000
ROWS, CPAD = FRAMES + 2, 128
REFLECT, ZERO_TAIL = 0, 1
F32 = np.float32

# the largest |fp32 restatement - float64| on the normalised log-mel over cases() at 80 and 128 mels, as test_mel_ref_cpu.py
# measures it (the test fails when this constant and its fresh figure differ by more than a factor of 2)
# 2.98e-5, on ragged(479999) / ragged(480000): among 3000 x n_mels values of plain noise a few one- or two-bin channels are small
# by chance, and the DFT's fp32 error is relative to the frame, not to the bin.  Impulses are at 1e-7, the tones at 1e-6 .. 2e-5
WORST_FP32 = 3.0e-5
# 32 x: the device's log10f (one ulp at -10 is 9.5e-7 before the division by 4), FMA contraction, another order inside the
# filterbank sum.  2e-4 is the project's stated front-end tolerance (test_gpu_parity.py) and the ceiling, which it reaches
TOL_MEL = min(2e-4, 32 * WORST_FP32)

MUTANTS = ("frame_shift", "hann_symmetric", "start_reflect", "end_reflect", "mode_swapped", "bin_step", "read_past_n",
           "neighbour_max", "previous_max", "chunks_no_plus1", "image_shift", "image_keeps_tail")
BIN_STEP_K = 37          # the bin the "bin_step" mutant computes with bin 38's twiddle step


def hann(mut=()):
    j = np.arange(N_FFT, dtype=np.float64)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * j / (N_FFT - 1 if "hann_symmetric" in mut else N_FFT))


def window_positions(n, mode, mut=(), stored=CHUNK):
    """[3000][400]: the sample of the window each (frame, j) reads, -1 where it reads a zero.  `stored`: how many samples lie
    behind the pointer (only the read_past_n mutant looks behind n)"""
    t = np.arange(FRAMES, dtype=np.int64)[:, None]
    j = np.arange(N_FFT, dtype=np.int64)[None, :]
    pos = HOP * t - N_FFT // 2 + j + (1 if "frame_shift" in mut else 0)
    pos = np.where(pos < 0, -pos - (1 if "start_reflect" in mut else 0), pos)
    if (mode ^ 1 if "mode_swapped" in mut else mode) == REFLECT:
        pos = np.where(pos >= CHUNK, 2 * (CHUNK if "end_reflect" in mut else CHUNK - 1) - pos, pos)
    else:
        pos = np.where(pos >= CHUNK, -1, pos)
    lim = min(stored, CHUNK) if "read_past_n" in mut else min(n, CHUNK)
    return np.where((pos >= 0) & (pos < lim), pos, -1)


def recording_positions(first, count, n):
    """[count][400] for frames first .. first + count - 1 of a recording of n samples"""
    t = first + np.arange(count, dtype=np.int64)[:, None]
    pos = HOP * t - N_FFT // 2 + np.arange(N_FFT, dtype=np.int64)[None, :]
    pos = np.where(pos < 0, -pos, pos)
    return np.where(pos < n, pos, -1)


def log_power(x, pos, filters, mut=()):
    """log10 of the mel power of the frames `pos` selects from x, before any clamp -> float64 [n_mels][frames]"""
    xz = np.concatenate([np.asarray(x, dtype=np.float64), [0.0]])          # index -1 reads the zero
    spec = np.fft.rfft(xz[pos] * hann(mut), axis=1)
    pw = spec.real ** 2 + spec.imag ** 2
    if "bin_step" in mut:
        pw[:, BIN_STEP_K] = pw[:, BIN_STEP_K + 1]
    mel = pw @ np.asarray(filters, dtype=np.float64).T
    return np.log10(np.maximum(mel, 1e-10)).T


def normalise(lm, mx):
    return (np.maximum(lm, mx - 8.0) + 4.0) / 4.0


def window_log_power(pcm, n, mode, filters, mut=()):
    pcm = np.asarray(pcm)
    n = min(int(n), CHUNK)
    lim = min(len(pcm), CHUNK) if "read_past_n" in mut else n
    return log_power(pcm[:lim], window_positions(n, mode, mut, stored=len(pcm)), filters, mut)


def log_mel_window(pcm, n, mode, filters, mut=()):
    """ohw_mel on one window: pcm[:n] (what lies behind n is never read) -> float64 [n_mels][3000]"""
    lm = window_log_power(pcm, n, mode, filters, mut)
    return normalise(lm, lm.max())


def recording_frames(n, mut=()):
    """how many frames the recording's maximum is taken over.  Frame t touches a sample when 160 t - 200 < n.  The library counts
    (n + 200) / 160 + 1 frames and rounds up to pseudo-windows of 3000; the mutant drops the + 1 of that count"""
    if "chunks_no_plus1" in mut:
        return -(-((n + N_FFT // 2) // HOP) // FRAMES) * FRAMES
    return (n + N_FFT // 2 - 1) // HOP + 1


def recording_log_power(pcm, filters, count=None):
    """frames 0 .. count - 1 of the whole recording, before the clamp -> float64 [n_mels][count]"""
    pcm = np.asarray(pcm)
    count = recording_frames(len(pcm)) if count is None else count
    out = np.empty((len(filters), count))
    for f0 in range(0, count, FRAMES):
        c = min(FRAMES, count - f0)
        out[:, f0:f0 + c] = log_power(pcm, recording_positions(f0, c, len(pcm)), filters)
    return out


def recording_max(pcm, filters, mut=()):
    """ohw_recording_set's result: the largest log10 mel power over the recording's frames, at least the -10 of its zero tail"""
    count = recording_frames(len(pcm), mut)
    return max(-10.0, float(recording_log_power(pcm, filters, count).max())) if count > 0 else -10.0


def log_mel_seek(pcm, seek, rec_max, filters):
    """ohw_mel_seek: frames seek .. seek + 2999 of the recording-wide spectrogram -> float64 [n_mels][3000]"""
    pcm = np.asarray(pcm)
    return normalise(log_power(pcm, recording_positions(int(seek), FRAMES, len(pcm)), filters), rec_max)


def round_16(a, dt):
    """fp32 -> the 16-bit type (dt 0 bf16, 1 f16) by one round-to-nearest-even conversion, widened back to fp32"""
    a = np.ascontiguousarray(a, dtype=F32)
    if dt == 1:
        return a.astype(np.float16).astype(F32)
    w = a.view(np.uint32).astype(np.uint64)
    w = (w + 0x7fff + ((w >> 16) & 1)) >> 16 << 16
    return w.astype(np.uint32).view(F32)


def image(mel_norm_fp32, n_mels, dt, t_lim=FRAMES, mut=()):
    """the time-major image conv1 reads, from the fp32 [n_mels][3000] the same call left -> fp32 [3002][128]"""
    m = np.asarray(mel_norm_fp32, dtype=F32)
    assert m.shape == (n_mels, FRAMES)
    img = np.zeros((ROWS, CPAD), dtype=F32)
    keep = FRAMES if "image_keeps_tail" in mut else min(int(t_lim), FRAMES)
    r0 = 0 if "image_shift" in mut else 1
    img[r0:r0 + keep, :n_mels] = round_16(m.T[:keep], dt)
    return img


# ---- the float32 restatement (tolerance only) ------------------------------------------------------------------------------
_memo = {}


def _fp32_power(x, pos):
    """|DFT|^2 of the windowed frames in float32 in mel_power_kernel's order -> [frames][201].  A frame of zeros has power 0
    exactly and is not run through the loop; a frame identical to the same row of the previous call (the two modes differ in
    one frame, the two filterbanks in none) is taken from that call"""
    xz = np.concatenate([np.asarray(x, dtype=F32), np.zeros(1, F32)])
    fr = xz[pos] * hann().astype(F32)
    pw = np.zeros((len(fr), N_FREQ), dtype=F32)
    todo = fr.any(axis=1)
    prev = _memo.get("last")
    if prev is not None and prev[0].shape == fr.shape:
        same = (prev[0] == fr).all(axis=1)
        pw[same] = prev[1][same]
        todo &= ~same
    rows = fr[todo]
    if len(rows):
        ang = 2.0 * np.pi * np.arange(N_FFT) / N_FFT
        cos, sin = np.cos(ang).astype(F32), np.sin(ang).astype(F32)
        k = np.arange(N_FREQ)
        idx = np.zeros(N_FREQ, dtype=np.int64)
        re = np.zeros((len(rows), N_FREQ), dtype=F32)
        im = np.zeros((len(rows), N_FREQ), dtype=F32)
        for j in range(N_FFT):
            col = rows[:, j:j + 1]
            re += col * cos[idx][None, :]
            im -= col * sin[idx][None, :]
            idx = (idx + k) % N_FFT
        pw[todo] = re * re + im * im
    _memo["last"] = (fr, pw)
    return pw


def _fp32_log_power(x, pos, filters):
    """log_power in float32: the power above, then the kernel's sequential 201-term filterbank dot and log10"""
    pw = _fp32_power(x, pos)
    filt = np.ascontiguousarray(np.asarray(filters, dtype=F32).T)                    # [201][n_mels]
    acc = np.zeros((len(pw), filt.shape[1]), dtype=F32)
    for k in range(N_FREQ):
        acc += pw[:, k:k + 1] * filt[k][None, :]
    return np.log10(np.maximum(acc, F32(1e-10))).T


def _fp32_normalise(lm, mx):
    return (np.maximum(lm, F32(mx) - F32(8.0)) + F32(4.0)) * F32(0.25)


def fp32_window(pcm, n, mode, filters):
    n = min(int(n), CHUNK)
    lm = _fp32_log_power(np.asarray(pcm)[:n], window_positions(n, mode), filters)
    return _fp32_normalise(lm, lm.max())


def fp32_recording(pcm, seeks, filters):
    """-> (the recording's maximum, the windows at `seeks`), all from one pass over the recording's frames"""
    pcm = np.asarray(pcm)
    count = recording_frames(len(pcm))
    lm = np.full((len(filters), max(count, max(seeks) + FRAMES)), F32(-10.0), dtype=F32)
    for f0 in range(0, count, FRAMES):
        c = min(FRAMES, count - f0)
        lm[:, f0:f0 + c] = _fp32_log_power(pcm, recording_positions(f0, c, len(pcm)), filters)
    mx = max(F32(-10.0), lm.max())
    return float(mx), [_fp32_normalise(lm[:, s:s + FRAMES], mx) for s in seeks]


def fp32_emulation(case, filters):
    """the float32 restatement of a Window or a Recording (at its seeks) -> list of [n_mels][3000] float32"""
    if isinstance(case, Window):
        return [fp32_window(case.pcm, case.n, case.mode, filters)]
    return fp32_recording(case.pcm, case.seeks, filters)[1]


def reference(case, filters):
    """the float64 reference of the same -> list of [n_mels][3000] float64"""
    if isinstance(case, Window):
        return [log_mel_window(case.pcm, case.n, case.mode, filters)]
    mx = recording_max(case.pcm, filters)
    return [log_mel_seek(case.pcm, s, mx, filters) for s in case.seeks]


# ---- the inputs ------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True, eq=False)
class Window:
    name: str
    pcm: np.ndarray          # 480000 samples as they lie in memory; only pcm[:n] may be read
    n: int
    mode: int


@dataclasses.dataclass(frozen=True, eq=False)
class Recording:
    name: str
    pcm: np.ndarray
    seeks: tuple


def _noise(tag, count, amp):
    return (amp * synth.uniform_pm1(synth.tensor_key(0x3E1, tag), 0, count)).astype(F32)


def _frozen(a):
    a = np.ascontiguousarray(a, dtype=F32)
    a.setflags(write=False)
    return a


IMPULSE_AT = (0, 1, 100, 159, 160, 199, 200, 201, 4000, 4079, 479480, 479800, 479900, 479999)
TONE_BINS = (1, 5, 37, 100, 199, 200)
RAGGED_N = (0, 1, 199, 200, 201, 479999, 480000)
MODES = (REFLECT, ZERO_TAIL)
MODE_NAMES = {REFLECT: "reflect", ZERO_TAIL: "zero_tail"}


@functools.lru_cache(maxsize=None)
def _impulse_pcm():
    x = np.zeros(CHUNK, F32)
    x[list(IMPULSE_AT)] = 0.7
    return _frozen(x)


def impulses(mode):
    """single samples of 0.7: each falls into 2 - 3 frames and sits on the Hann window's slope in at least one of them"""
    return Window(f"impulses/{MODE_NAMES[mode]}", _impulse_pcm(), CHUNK, mode)


@functools.lru_cache(maxsize=None)
def _tone_pcm(k, amp=0.5):
    t = np.arange(CHUNK, dtype=np.float64) / 16000.0
    return _frozen(amp * np.sin(2.0 * np.pi * 40.0 * k * t + 0.3))


def bin_tone(k, mode=REFLECT):
    """a tone on the centre of DFT bin k (the bins are 40 Hz wide): under the periodic window its energy lies in bins k - 1 .. k + 1"""
    return Window(f"bin_tone{k}/{MODE_NAMES[mode]}", _tone_pcm(k), CHUNK, mode)


@functools.lru_cache(maxsize=None)
def _ragged_pcm(n):
    x = _noise("ragged", CHUNK, 1.0).copy()      # the same noise for every n: what lies in [n, 480000) is full scale ...
    x[:n] *= F32(0.1)                            # ... and ten times what may be read
    return _frozen(x)


def ragged(n, mode=REFLECT):
    return Window(f"ragged{n}/{MODE_NAMES[mode]}", _ragged_pcm(n), n, mode)


@functools.lru_cache(maxsize=None)
def _triplet_pcm():
    return (_tone_pcm(25, 1.0), _frozen(_noise("quiet", CHUNK, 1e-3)), _frozen(np.zeros(CHUNK, F32)))


def loudness_triplet(mode=REFLECT):
    """three windows of one batch: a full-scale tone (positive maximum), noise of 1e-3 (negative maximum), exact silence"""
    return [Window(f"triplet_{what}/{MODE_NAMES[mode]}", x, CHUNK, mode) for what, x in zip(("tone", "noise", "silence"), _triplet_pcm())]


REC_A_N = 2 * CHUNK + 12345
REC_A_SEEKS = (0, 2995, 3000, 3005, 5990, 7000)      # 7000: every frame lies in the zero tail behind the recording


@functools.lru_cache(maxsize=None)
def recording_a():
    """noise of 0.02 over two windows and a bit, 20000 samples of exact silence in the first window (where the burst's clamp shows:
    alone, that window would clamp 2 lower), a burst of 0.9 noise only inside the second window, impulses 50 samples before and
    behind the window boundary"""
    x = _noise("rec_a", REC_A_N, 0.02).copy()
    x[100000:120000] = 0.0
    x[CHUNK + 200000:CHUNK + 208000] = _noise("rec_a_burst", 8000, 0.9)
    x[CHUNK - 50] = 0.7
    x[CHUNK + 50] = 0.7
    return Recording("recording_a", _frozen(x), REC_A_SEEKS)


# silence except one impulse of 0.5 at the last sample.  The library's pseudo-window count changes between n = 479799 (one) and
# 479800 (two).  At 479800 and 479801 the second pseudo-window's only frame, 3000, starts at sample 479800, where the Hann
# window is 0 or the sample is absent: it sees nothing.  At 479959 the impulse is at j = 158 of frame 3000, j = 318 of frame
# 2999 and j = 478 of frame 2998: frame 3000 is the loudest of the recording, and only the second pseudo-window holds it
REC_B_N = (CHUNK - 199, CHUNK - 200, CHUNK - 201, CHUNK - 41)


@functools.lru_cache(maxsize=None)
def recording_b(n):
    x = np.zeros(n, F32)
    x[n - 1] = 0.5
    return Recording(f"recording_b{n}", _frozen(x), (0, (n - 1) // HOP - 1))


@functools.lru_cache(maxsize=None)
def recording_c():
    """-> (loud, quiet): set one after the other on the same state.  The quiet one has a stretch of silence: under the loud
    recording's maximum its noise would clamp, under its own only the silence does"""
    loud = _noise("rec_c_loud", CHUNK + 5000, 0.8)
    quiet = _noise("rec_c_quiet", CHUNK - 7777, 1e-3).copy()
    quiet[300000:310000] = 0.0
    return Recording("recording_c_loud", _frozen(loud), (0, 20)), Recording("recording_c_quiet", _frozen(quiet), (0, 1000))


def cases():
    """every builder input, in the order that lets the float32 restatement reuse what two neighbours share"""
    out = []
    for m in MODES:
        out.append(impulses(m))
    for k in TONE_BINS:
        out += [bin_tone(k, m) for m in MODES]
    for n in RAGGED_N:
        out += [ragged(n, m) for m in MODES]
    trip = [loudness_triplet(m) for m in MODES]
    for b in range(3):
        out += [trip[0][b], trip[1][b]]
    out.append(recording_a())
    out += [recording_b(n) for n in REC_B_N]
    out += list(recording_c())
    return out
