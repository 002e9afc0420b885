"""The speech plan on the host (ohw_speech_segments_host, ohw_speech_chunks_host: csrc/vad.cpp) against the restatement of
tests/vad_ref.py: seeded random probability tracks, hand cases at every edge of the two rules, the injected faults of
vad_ref.MUTANTS (each must be flagged by a hand case, which is what makes them cases), the chunk invariants, and the detector
rule itself in float64 on the synthetic audio the GPU tests use.  No GPU."""
import numpy as np
import pytest

import vad_ref as R
from openhush_amd import engine as E

F32 = np.float32


def c_config(cfg):
    return E.VadConfig(0, cfg.threshold, cfg.min_silence_ms, cfg.min_speech_ms, cfg.speech_pad_ms)


def c_plan(pl):
    return E.ChunkPlan(pl.max_chunk_s, pl.max_gap_ms, pl.min_chunk_ms)


def lib_segments(p, fs, n, cfg):
    return E.speech_segments_host(p, fs, n, c_config(cfg))


def lib_chunks(segs, p, fs, n, pl):
    return E.speech_chunks_host(segs, p, fs, n, c_plan(pl))


def random_track(rng, n_frames):
    """speech and silence runs of random lengths, a level per run, noise on top: thresholds, pending ends and pads all get hit"""
    p = np.empty(n_frames, dtype=F32)
    f = 0
    while f < n_frames:
        ln = int(rng.choice([1, 2, 5, 20, 60, 150, 400, 3500]))
        level = float(rng.choice([0.02, 0.2, 0.36, 0.45, 0.55, 0.9]))
        p[f:f + ln] = np.clip(level + rng.normal(0, 0.05, size=len(p[f:f + ln])), 0, 1)
        f += ln
    return p


def check_invariants(ch, segs, cuts, n, pl):
    max_len, min_chunk = int(float(F32(pl.max_chunk_s)) * 16000.0), pl.min_chunk_ms * 16
    for c, (a, b, first, cnt) in enumerate(ch):
        assert 0 <= a < b <= n and b - a <= max_len and cnt >= 1
        if c > 0:
            assert a >= ch[c - 1][1]                                               # ordered and disjoint
        room_l = a - (ch[c - 1][1] if c > 0 else 0)
        room_r = (ch[c + 1][0] if c + 1 < len(ch) else n) - b
        # at least min_chunk unless the recording is shorter - or, the rule's own bound, no room is left on either side
        assert b - a >= min(min_chunk, n) or (room_l == 0 and room_r == 0), (c, a, b)
    for i, sg in enumerate(segs):
        holders = [c for c in ch if c[0] <= sg[0] and sg[1] <= c[1]]
        if holders:
            assert len(holders) == 1
        else:                                                                          # cut: the pieces tile it, joined at stated cuts
            pieces = [c for c in ch if c[2] <= i < c[2] + c[3] and c[1] > sg[0] and c[0] < sg[1]]
            assert len(pieces) >= 2 and pieces[0][0] <= sg[0] and pieces[-1][1] >= sg[1]
            for x, y in zip(pieces, pieces[1:]):
                assert x[1] == y[0] and x[1] in cuts


@pytest.mark.parametrize("fs", [160, 512])
def test_random_tracks_match_the_restatement(fs):
    rng = np.random.default_rng(20 + fs)
    for case in range(150):
        n_frames = int(rng.integers(1, 9000 if case % 10 else 30000))
        p = random_track(rng, n_frames)
        n = n_frames * fs - int(rng.integers(0, fs))
        cfg = R.config(threshold=float(rng.choice([0.3, 0.5, 0.7])), min_silence_ms=int(rng.choice([100, 700, 2000])),
                       min_speech_ms=int(rng.choice([0, 250, 1000])), speech_pad_ms=int(rng.choice([0, 30, 400])))
        pl = R.plan(max_chunk_s=float(rng.choice([5.0, 12.5, 30.0])), max_gap_ms=int(rng.choice([0, 500, 2000])),
                    min_chunk_ms=int(rng.choice([0, 1100, 3000])))
        want = R.segments(p, fs, n, cfg)
        got = lib_segments(p, fs, n, cfg)
        assert got == want, (case, fs)
        cuts = []
        want_ch = R.chunks(want, p, fs, n, pl, cuts_out=cuts)
        assert lib_chunks(got, p, fs, n, pl) == want_ch, (case, fs)
        check_invariants(want_ch, want, cuts, n, pl)


def track(n_frames, runs, low=0.02):
    p = np.full(n_frames, low, dtype=F32)
    for a, b, v in runs:
        p[a:b] = v
    return p


# name -> (probabilities, frame_samples, n_samples, config, plan)
def hand_cases():
    d = {}
    d["speech_to_the_last_frame"] = (track(500, [(300, 500, 0.9)]), 160, 80000, R.config(), R.plan())
    # min_silence 700 ms = 70 frames: the pending end at 200 is cancelled by speech at frame 268, one frame before the 70th
    d["pending_end_cancelled_one_frame_early"] = (track(700, [(100, 200, 0.9), (269, 400, 0.9)]), 160, 112000, R.config(), R.plan())
    d["pending_end_kept_at_min_silence"] = (track(700, [(100, 200, 0.9), (270, 400, 0.9)]), 160, 112000, R.config(), R.plan())
    d["one_frame_under_min_speech"] = (track(400, [(100, 124, 0.9), (250, 275, 0.9)]), 160, 64000, R.config(min_silence_ms=100), R.plan())
    # two segments 11 frames apart with pads of 400 ms: they meet at the gap's midpoint; the first pad is clipped at 0 and the
    # last at n_samples
    d["pads_meet_at_a_midpoint"] = (track(300, [(10, 100, 0.9), (111, 290, 0.9)]), 160, 47990, R.config(min_silence_ms=100, speech_pad_ms=400), R.plan())
    # between neg and the threshold: no pending end is set by 0.4 (neg = 0.35), so the segment runs on
    d["between_neg_and_threshold"] = (track(600, [(100, 200, 0.9), (200, 400, 0.4), (400, 450, 0.9)]), 160, 96000, R.config(), R.plan())
    p = track(7300, [(100, 7100, 0.9)])
    p[2500], p[2600], p[5000] = 0.6, 0.6, 0.55                                # the first of two equal minima; then a single one
    d["a_70_s_segment_cut_twice"] = (p, 160, 7300 * 160, R.config(), R.plan())
    d["short_segment_grown_against_the_start"] = (track(1000, [(5, 35, 0.9)]), 160, 160000, R.config(min_silence_ms=100), R.plan())
    d["zero_segments"] = (track(1000, []), 160, 160000, R.config(), R.plan())
    d["frame_samples_512"] = (track(400, [(20, 90, 0.9), (130, 180, 0.9), (300, 330, 0.9)]), 512, 400 * 512 - 100, R.config(), R.plan(max_gap_ms=1000))
    return d


CASES = hand_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_cases(name):
    p, fs, n, cfg, pl = CASES[name]
    want = R.segments(p, fs, n, cfg)
    assert lib_segments(p, fs, n, cfg) == want
    cuts = []
    want_ch = R.chunks(want, p, fs, n, pl, cuts_out=cuts)
    assert lib_chunks(want, p, fs, n, pl) == want_ch
    check_invariants(want_ch, want, cuts, n, pl)


def test_hand_cases_say_what_they_are_built_for():
    seg = {k: R.segments(v[0], v[1], v[2], v[3]) for k, v in CASES.items()}
    ch = {k: R.chunks(seg[k], v[0], v[1], v[2], v[4]) for k, v in CASES.items()}
    assert seg["speech_to_the_last_frame"] == [(300 * 160 - 480, 80000, pytest.approx(0.9))]
    assert len(seg["pending_end_cancelled_one_frame_early"]) == 1 and len(seg["pending_end_kept_at_min_silence"]) == 2
    assert seg["pending_end_kept_at_min_silence"][0][:2] == (100 * 160 - 480, 200 * 160 + 480)
    assert [s[:2] for s in seg["one_frame_under_min_speech"]] == [(250 * 160 - 480, 275 * 160 + 480)]
    a, b = seg["pads_meet_at_a_midpoint"]
    assert a[0] == 0 and a[1] == b[0] == 100 * 160 + (11 * 160) // 2 and b[1] == 47990
    assert len(seg["between_neg_and_threshold"]) == 1
    assert [c[:2] for c in ch["a_70_s_segment_cut_twice"]] == [(100 * 160 - 480, 2500 * 160), (2500 * 160, 5000 * 160), (5000 * 160, 7100 * 160 + 480)]
    assert ch["short_segment_grown_against_the_start"] == [(0, 1100 * 16, 0, 1)]
    assert seg["zero_segments"] == [] and ch["zero_segments"] == []
    assert len(seg["frame_samples_512"]) == 3 and [c[2:] for c in ch["frame_samples_512"]] == [(0, 1), (1, 1), (2, 1)]
    assert E.speech_chunks_host([], CASES["zero_segments"][0], 160, 160000) == []


@pytest.mark.parametrize("mut", R.MUTANTS)
def test_every_injected_fault_is_flagged_by_a_hand_case(mut):
    flagged = []
    for name, (p, fs, n, cfg, pl) in CASES.items():
        good = R.segments(p, fs, n, cfg)
        bad = R.segments(p, fs, n, cfg, mut=(mut,))
        if bad != good or R.chunks(good, p, fs, n, pl, mut=(mut,)) != R.chunks(good, p, fs, n, pl):
            flagged.append(name)
            # and the library sides with the rule, not with the fault
            assert lib_segments(p, fs, n, cfg) == good and lib_chunks(good, p, fs, n, pl) == R.chunks(good, p, fs, n, pl)
    assert flagged, mut


def test_defaults_and_refusals():
    c, d, p = E.default_vad_config(), E.default_vad_detector(), E.default_chunk_plan()
    assert (c.threshold, c.min_silence_ms, c.min_speech_ms, c.speech_pad_ms) == (0.5, 700, 250, 30)
    assert (round(d.floor_quantile, 6), d.margin_db, d.slope_db) == (0.1, 9.0, 3.0)
    assert (p.max_chunk_s, p.max_gap_ms, p.min_chunk_ms) == (30.0, 2000, 1100)
    # the batch path drops a cut of at most 100 frames of 10 ms (TranscribeCall::decode_windows): the default stays above it
    assert p.min_chunk_ms > 1000 + 25                      # 1 s, and the 200-sample margin of the frame count
    z = np.zeros(10, F32)
    with pytest.raises(ValueError):
        E.speech_segments_host(z, 0, 1600)
    with pytest.raises(ValueError):
        E.speech_chunks_host([(0, 100)], z, 160, 1600, E.ChunkPlan(31.0, 2000, 1100))
    with pytest.raises(ValueError):
        E.speech_chunks_host([(100, 50)], z, 160, 1600)


def test_detector_rule_in_float64_finds_the_bursts():
    """the rule's own check (float64, defaults): 12.3 s of noise at -60 dBFS with three modulated four-tone bursts at -20 dBFS;
    every unpadded segment edge within 30 ms of the truth"""
    bursts = [(1.0, 3.2), (5.0, 6.5), (8.9, 11.4)]
    x = R.burst_audio(12.3, bursts)
    n = len(x)
    e = R.band_energy(x, n)
    fl = R.floor32(e.astype(F32), 0.10)
    p, _ = R.probs64(e, fl, 9.0, 3.0)
    raw = R.raw_segments(p.astype(F32), 160, R.config())
    assert len(raw) == len(bursts)
    for (f0, f1), (t0, t1) in zip(raw, bursts):
        assert abs(f0 - round(t0 * 100)) <= 3 and abs(f1 - round(t1 * 100)) <= 3, (f0, f1, t0, t1)      # in frames of 10 ms
