"""The speech-aware front half (csrc/vad.hip, the plan in csrc/vad.cpp) restated in numpy: the detector's three rules in float64,
float32 replicas of the histogram's binning and quantile step (integers and one fp32 product: those compare EXACTLY), the
segment and chunk rules on integers, the error bounds of the GPU tests - derived here from the number formats alone, never
from what the kernels give - and the synthetic audio the tests share.  All three rules are this project's own (include/ohw.h).

  band    frame t = 400 samples centred at 160 t under the periodic Hann window, reflected at the recording's start only, zero
          from n on; e[t] = 10 log10(max(sum_{k=8..85} |X_t[k]|^2, 1e-10))
  floor   bin = clamp(floor((e + 100) * 2), 0, 319); the floor is the lower edge of the first bin whose cumulative count reaches
          ceil(q * n_frames)
  prob    es[t] = mean of e over the frames of [t - 2, t + 2] that exist; p = 1 / (1 + exp(-(es - floor - margin) / slope))

MUTANTS are mistakes a restatement could make; tests/test_vad_ref_cpu.py shows that the hand cases flag every one of them."""
import math
from types import SimpleNamespace

import numpy as np

N_FFT, HOP = 400, 160
K0, K1 = 8, 85
BINS = 320
F32 = np.float32
U = 2.0 ** -24                   # fp32 unit roundoff

MUTANTS = ("neg_is_threshold", "end_at_current", "pads_unclipped", "cut_last_min")


def n_frames_of(n):
    return (n + HOP - 1) // HOP


# ---- band energy ------------------------------------------------------------------------------------------------------------
def hann():
    j = np.arange(N_FFT, dtype=np.float64)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * j / N_FFT)


def windowed_frames(pcm, n):
    """[n_frames][400] float64: only pcm[:n] counts, whatever lies behind it"""
    x = np.concatenate([np.asarray(pcm[:n], dtype=np.float64), np.zeros(1)])
    t = np.arange(n_frames_of(n))[:, None]
    pos = t * HOP - N_FFT // 2 + np.arange(N_FFT)[None, :]
    pos = np.abs(pos)                                   # reflected at the start only
    pos = np.where(pos < n, pos, n)                     # zero from n on
    return x[pos] * hann()[None, :]


def band_power(fr):
    """sum of |X[k]|^2 over k = 8..85, float64"""
    k = np.arange(K0, K1 + 1)
    ang = 2.0 * np.pi * np.outer(np.arange(N_FFT), k) / N_FFT
    re = fr @ np.cos(ang)
    im = -(fr @ np.sin(ang))
    return (re * re + im * im).sum(axis=1)


def band_energy(pcm, n):
    return 10.0 * np.log10(np.maximum(band_power(windowed_frames(pcm, n)), 1e-10))


# what log10f and the product by 10 add, in dB: log10f within 2 ulp of a value below 16 (ulp 9.5e-7), the product rounded once at
# a magnitude below 128 (half an ulp: 3.8e-6)
LOG_ERR_DB = 10 * 2 * 2.0 ** -20 + 2.0 ** -18


def energy_tolerance(pcm, n):
    """per frame, in dB: the worst case of fp32 accumulation of a 400-term DFT.  re and im are each a sequential sum of 400
    products x[j] w[j] c[j] of rounded factors: |d re| <= gamma_403 * S with S = sum |x[j] w[j]| (Higham 3.5; 400 additions, the
    window, twiddle and product roundings), so |dX| <= a = sqrt(2) * 403 u S.  A bin's power moves by at most 2 |X| a + a^2 (+ 3
    roundings), the 78-term band sum P by dP <= 2 a sqrt(78 P) + 78 a^2 + 82 u P (Cauchy-Schwarz; gamma_78 and the squares).
    The error is relative to the FRAME (S), not to the band: a frame with little in-band power has a wide bound, honestly.  In dB:
    the distance from 10 log10(max(P, 1e-10)) to the same of P +- dP, plus LOG_ERR_DB."""
    fr = windowed_frames(pcm, n)
    P = band_power(fr)
    S = np.abs(fr).sum(axis=1)
    a = math.sqrt(2.0) * 403 * U * S
    dP = 2.0 * a * np.sqrt(78.0 * P) + 78.0 * a * a + 82 * U * P

    def db(v):
        return 10.0 * np.log10(np.maximum(v, 1e-10))
    return np.maximum(db(P + dP) - db(P), db(P) - db(P - dP)) + LOG_ERR_DB


# ---- floor: float32 replicas, compared exactly ------------------------------------------------------------------------------
def bins32(e):
    e = np.asarray(e, dtype=F32)
    with np.errstate(over="ignore", invalid="ignore"):
        b = np.floor((e + F32(100.0)) * F32(2.0))
    return np.clip(b, F32(0.0), F32(BINS - 1)).astype(np.int64)


def target32(q, n_frames):
    t = int(np.ceil(F32(q) * F32(n_frames)))
    return min(max(t, 1), n_frames)


def floor32(e, q):
    """the noise floor in dB (a multiple of 0.5: exact in fp32)"""
    hist = np.bincount(bins32(e), minlength=BINS)
    cum = np.cumsum(hist)
    b = int(np.argmax(cum >= target32(q, len(e))))
    return -100.0 + 0.5 * b


# ---- probability --------------------------------------------------------------------------------------------------------------
def smoothed(e):
    e = np.asarray(e, dtype=np.float64)
    n = len(e)
    out = np.empty(n)
    for t in range(n):
        a, b = max(t - 2, 0), min(t + 2, n - 1)
        out[t] = e[a:b + 1].sum() / (b - a + 1)
    return out


def probs64(e, floor_db, margin_db, slope_db):
    z = (smoothed(e) - floor_db - float(F32(margin_db))) / float(F32(slope_db))
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-z)), z


def prob_tolerance(z, slope_db):
    """|p_fp32 - p| for e given in fp32.  z: the 5-term mean (values within +-160: gamma_6 * 160 = 5.7e-5), less the floor and the
    margin (two roundings at a magnitude below 512: 6.1e-5), over the slope (one rounding): |dz| <= 1.2e-4 / slope + 2 u |z|.
    The device's expf is within 2 ulp, so exp(-z) is off by a factor of (1 +- (|dz| + 2 u)) and p by p (1 - p) <= 1/4 of that;
    1 + x and the reciprocal add 2 roundings of p <= 1.  A p below the smallest normal number may come out as 0."""
    dz = 1.2e-4 / slope_db + 2 * U * np.abs(z)
    return 0.25 * (dz + 4 * U) + 4 * U + 1.2e-38


# ---- the plan -----------------------------------------------------------------------------------------------------------------
def config(threshold=0.5, min_silence_ms=700, min_speech_ms=250, speech_pad_ms=30):
    return SimpleNamespace(threshold=threshold, min_silence_ms=min_silence_ms, min_speech_ms=min_speech_ms, speech_pad_ms=speech_pad_ms)


def plan(max_chunk_s=30.0, max_gap_ms=2000, min_chunk_ms=1100):
    return SimpleNamespace(max_chunk_s=max_chunk_s, max_gap_ms=max_gap_ms, min_chunk_ms=min_chunk_ms)


def raw_segments(probs, fs, cfg, mut=()):
    """[(first frame, end frame)] before the pads"""
    p = np.asarray(probs, dtype=F32)
    thr = F32(cfg.threshold)
    neg = thr if "neg_is_threshold" in mut else max(thr - F32(0.15), F32(0.01))
    min_silence, min_speech = cfg.min_silence_ms * 16, cfg.min_speech_ms * 16
    out, start, pending = [], None, None
    for f in range(len(p)):
        if p[f] >= thr:
            if start is None:
                start = f
            pending = None
        elif start is not None:
            if p[f] < neg and pending is None:
                pending = f
            if pending is not None and (f + 1 - pending) * fs >= min_silence:
                end = f if "end_at_current" in mut else pending
                if (end - start) * fs >= min_speech:
                    out.append((start, end))
                start = pending = None
    if start is not None and (len(p) - start) * fs >= min_speech:
        out.append((start, len(p)))
    return out


def segments(probs, fs, n_samples, cfg, mut=()):
    """[(start, end, avg_probability)] in samples"""
    raw = raw_segments(probs, fs, cfg, mut)
    pad = cfg.speech_pad_ms * 16
    out = []
    for i, (f0, f1) in enumerate(raw):
        a, b = f0 * fs - pad, f1 * fs + pad
        if i > 0:
            gap = f0 * fs - raw[i - 1][1] * fs
            if gap < 2 * pad:
                a = raw[i - 1][1] * fs + gap // 2
        if i + 1 < len(raw):
            gap = raw[i + 1][0] * fs - f1 * fs
            if gap < 2 * pad:
                b = f1 * fs + gap // 2
        if "pads_unclipped" not in mut:
            a, b = min(max(a, 0), n_samples), min(max(b, 0), n_samples)
        s = 0.0
        for f in range(f0, f1):                       # the library's order: one double sum, front to back
            s += float(probs[f])
        out.append((a, b, float(F32(s / (f1 - f0)))))
    return out


def chunks(segs, probs, fs, n_samples, pl, mut=(), cuts_out=None):
    """[(start, end, first_segment, n_segments)]; cuts_out collects the samples where a long segment was cut"""
    p = np.asarray(probs, dtype=F32)
    max_len = int(float(F32(pl.max_chunk_s)) * 16000.0)
    max_gap, min_chunk = pl.max_gap_ms * 16, pl.min_chunk_ms * 16
    ch, cur, prev_end = [], None, 0
    for i, sg in enumerate(segs):
        s, e = sg[0], sg[1]
        if cur is not None and (s - prev_end > max_gap or e - cur[0] > max_len):
            ch.append(cur)
            cur = None
        if cur is None:
            while e - s > max_len:
                lo, hi = s + max_len // 2, s + max_len
                f0 = -(-lo // fs)
                f1 = min(len(p), -(-hi // fs))              # frames with f * fs < hi
                cut = hi
                if f1 > f0:
                    w = p[f0:f1]
                    k = (len(w) - 1 - int(np.argmin(w[::-1]))) if "cut_last_min" in mut else int(np.argmin(w))
                    cut = (f0 + k) * fs
                ch.append([s, cut, i, 1])
                if cuts_out is not None:
                    cuts_out.append(cut)
                s = cut
            cur = [s, e, i, 1]
        else:
            cur[1] = e
            cur[3] += 1
        prev_end = e
    if cur is not None:
        ch.append(cur)
    for c, k in enumerate(ch):
        need = min_chunk - (k[1] - k[0])
        if need <= 0:
            continue
        avail_l = k[0] - (ch[c - 1][1] if c > 0 else 0)
        avail_r = (ch[c + 1][0] if c + 1 < len(ch) else n_samples) - k[1]
        a = min(need // 2, avail_l)
        b = min(need - a, avail_r)
        a = min(need - b, avail_l)
        k[0] -= a
        k[1] += b
    return [tuple(k) for k in ch]


# ---- audio the tests share: noise at -60 dBFS, amplitude-modulated four-tone bursts at -20 dBFS at known times ------------------
TONES_HZ = (440.0, 880.0, 1320.0, 2200.0)


def burst_audio(seconds, bursts, seed=7, dips=()):
    """-> float32 [seconds * 16000].  bursts: [(t0, t1)] in seconds, on multiples of 10 ms.  The modulation (4 Hz, depth 0.3) keeps
    a burst well above the threshold throughout.  dips: [(t0, t1)] where a burst falls to the noise (a planted pause)"""
    n = int(round(seconds * 16000))
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n) * 1e-3                      # -60 dBFS rms
    t = np.arange(n) / 16000.0
    tone = sum(np.sin(2 * np.pi * f * t + 0.3 * i) for i, f in enumerate(TONES_HZ)) / len(TONES_HZ)
    tone *= 0.1 * math.sqrt(2.0 * len(TONES_HZ)) * (1.0 + 0.3 * np.sin(2 * np.pi * 4.0 * t)) / 1.3      # about -20 dBFS rms
    gate = np.zeros(n)
    for a, b in bursts:
        gate[int(round(a * 16000)):int(round(b * 16000))] = 1.0
    for a, b in dips:
        gate[int(round(a * 16000)):int(round(b * 16000))] = 0.0
    return (x + tone * gate).astype(F32)
