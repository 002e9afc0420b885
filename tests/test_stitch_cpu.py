"""Stitched windows without a GPU: the restatement against transformers' _find_longest_common_sequence, the host seam rule
against the restatement word for word, the window plan, the range and clip rules, and the faults the word comparison has to flag
on the shared table (tests/stitch_ref.py)."""
import numpy as np
import pytest

import stitch_ref as S
from openhush_amd import engine as E

EOT = 50257


@pytest.fixture(scope="module")
def table():
    return S.table()


def _random_pairs(n, seed):
    rng = np.random.default_rng(seed)
    for k in range(n):
        L, R = int(rng.integers(0, 70)), int(rng.integers(0, 70))
        kind = k % 4
        if kind == 0:                                            # a small alphabet: many accidental matches and near ties
            yield [int(x) for x in rng.integers(0, 4, L)], [int(x) for x in rng.integers(0, 4, R)]
        elif kind == 1:
            yield [int(x) for x in rng.integers(0, 50000, L)], [int(x) for x in rng.integers(0, 50000, R)]
        else:                                                    # a planted overlap with a few mismatches
            left = [int(x) for x in rng.integers(0, 50000, L)]
            ov = int(rng.integers(0, min(L, R) + 1))
            right = left[L - ov:] + [int(x) for x in rng.integers(0, 50000, R - ov)]
            for _ in range(int(rng.integers(0, 3))):
                if right:
                    right[int(rng.integers(0, len(right)))] = 50001
            yield left, right


def test_the_restatement_is_transformers_merge_on_pairs():
    tw = pytest.importorskip("transformers.models.whisper.tokenization_whisper")
    pairs = [(a, b) for _, a, b in S.cases()] + list(_random_pairs(2000, 5))
    assert len(pairs) >= 2150
    for a, b in pairs:
        assert tw._find_longest_common_sequence([a, b]) == S.merge_pair(a, b), (a, b)


def test_the_host_rule_equals_the_restatement_word_for_word(table):
    tok, n_text, names, want = table
    got = E.stitch_seams_host((tok, n_text))
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, [(int(s), names[s // 2] if s % 2 == 0 else "between", got[s].tolist(), want[s].tolist()) for s in bad[:5]]
    assert got.shape == (299, 8)
    # lists of ids, without a table: the random pairs
    for a, b in _random_pairs(300, 11):
        assert E.stitch_seams_host([a, b]).tolist() == S.seams([a, b], None).tolist()
    # the named properties of the table
    by = {n: want[2 * k] for k, n in enumerate(names)}
    assert by["tie 100/200"][1:3].tolist() == [100, 2] and by["tie 50/400"][1:3].tolist() == [50, 2] and by["tie 125/160"][1:3].tolist() == [125, 2]
    assert by["one match only"][1:5].tolist() == [0, 0, 120, 0] and by["L0R0"][1:7].tolist() == [0, 0, 0, 0, 0, 0]
    assert by["period 3"][1:3].tolist() == [90, 90] and by["R inside L"][1] > by["R inside L"][6] and by["L inside R"][1] > by["L inside R"][5]
    assert by["fp32 picks another shift"][1:3].tolist() == [200, 16]


def test_one_window_or_none_has_no_seam():
    assert E.stitch_seams_host([[1, 2, 3]]).shape == (0, 8) and E.stitch_seams_host([]).shape == (0, 8)
    with pytest.raises(E.WhisperError):
        E.stitch_seams_host((np.zeros((2, 8), np.int32), np.array([3, 9], np.int32)))      # a count past the stride


FAULTS = {
    "one match accepted": dict(min_matches=1),
    ">= in place of >": dict(strict=False),
    "eps dropped": dict(eps=False),
    "le not clipped": dict(clip_le=False),
    "re not clipped": dict(clip_re=False),
    "a read at tokens[n_text]": dict(overread=1),
    "midpoint rounded up": dict(round_up=True),
    "fp32 score": dict(dtype=np.float32),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_the_word_comparison_flags_an_injected_fault(table, fault):
    """the table is the first 60 windows here (every designed case); the fp32 fault stands for the search the issue asks for:
    among all (matches, shift) with L = R = 448 there are 363 neighbouring pairs that float64 and fp32 order differently, the
    smallest being 9 matches at shift 100 (0.09999999999999999) under 16 at shift 200 (0.1), which fp32 turns round (0.1 above
    0.099999994) - the case "fp32 picks another shift" of the table"""
    tok, n_text, names, want = table
    n = 60
    faulty = S.seams(tok[:n], n_text[:n], **FAULTS[fault])
    hit = np.flatnonzero((faulty != want[:n - 1]).any(axis=1))
    assert hit.size > 0, fault
    if fault == "fp32 score":
        assert 2 * names.index("fp32 picks another shift") in hit.tolist()
        assert np.float32(9) / np.float32(100) + np.float32(100) / np.float32(10000) > np.float32(16) / np.float32(200) + np.float32(200) / np.float32(10000)
        assert 9 / 100 + 100 / 10000.0 < 16 / 200 + 200 / 10000.0


def test_the_plan_covers_the_recording_and_the_last_window_reaches_past_the_one_before():
    rng = np.random.default_rng(3)
    sizes = [1, 479999, 480000, 480001, 880000, 880001, 960000, 57600000] + [int(x) for x in rng.integers(1, 6000000, 60)]
    for ms in (0, 1000, 1020, 5000, 14980, 15000):
        for n in sizes:
            hop, w = E.stitch_plan_host(n, ms)
            assert (hop, w) == S.plan(n, ms)[:2] and hop == 480000 - 16 * ms
            spans = S.plan(n, ms)[2]
            assert spans[0][0] == 0 and spans[-1][1] == n                              # the windows cover the recording
            for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
                assert b0 <= a1 and b0 < b1 and b1 > a1                                 # no gap; every window reaches past the one before
                assert a1 - a0 == 480000                                               # every window but the last is full
            if ms == 0:
                assert w == -(-n // 480000)
            if w > 1:
                assert (w - 2) * hop + 480000 < n                                      # one window fewer would not cover it
    assert E.stitch_plan_host(0, 0) == (480000, 0)
    for bad in (-20, 20, 980, 999, 1010, 5001, 15020, 30000):
        with pytest.raises(E.WhisperError):
            E.stitch_plan_host(1000000, bad)


def test_the_ranges_on_hand_cases():
    # three windows of 10, 8 and 6 text tokens: seam 0 cuts at (7, 2), seam 1 at (5, 1)
    seams = np.array([[0, 5, 4, 7, 2, 10, 8, 0], [1, 3, 3, 5, 1, 8, 6, 0]], np.int32)
    assert E.stitch_ranges_host(seams, [10, 8, 6]) == [(0, 7), (2, 5), (1, 6)] == S.ranges(seams, [10, 8, 6])
    # rc > lc: the middle window contributes nothing, its range is empty at rc
    seams = np.array([[0, 9, 8, 6, 6, 10, 8, 0], [1, 7, 7, 2, 3, 8, 6, 0]], np.int32)
    assert E.stitch_ranges_host(seams, [10, 8, 6]) == [(0, 6), (6, 6), (3, 6)] == S.ranges(seams, [10, 8, 6])
    # unmatched seams keep both windows whole; one window keeps everything
    seams = np.array([[0, 0, 0, 10, 0, 10, 8, 0]], np.int32)
    assert E.stitch_ranges_host(seams, [10, 8]) == [(0, 10), (0, 8)]
    assert E.stitch_ranges_host(np.zeros((0, 8), np.int32), [4]) == [(0, 4)]
    # in kept positions: timestamps of an uncut end stay, a cut end starts or stops at the text token itself
    ts = 50364
    win = [ts, 11, 12, ts + 50, ts + 50, 13, 14, ts + 100]
    assert S.kept_range(win, 0, 4, EOT) == (0, 8) and S.kept_range(win, 0, 2, EOT) == (0, 5) and S.kept_range(win, 2, 4, EOT) == (5, 8)
    assert S.kept_range(win, 1, 3, EOT) == (2, 6) and S.kept_range(win, 4, 4, EOT) == (8, 8) and S.kept_range(win, 3, 3, EOT) == (6, 6)
    assert S.kept_range([ts, ts + 10], 0, 0, EOT) == (0, 2)


def test_the_segment_clip_on_hand_cases():
    seg = (2, 9, 31.0, 36.5)
    for first, end, tl, tr in [(0, 20, 30.0, 40.0), (2, 9, 33.0, 34.0), (4, 20, 33.0, 40.0), (4, 20, 29.0, 40.0), (4, 20, 37.0, 40.0),
                               (0, 6, 30.0, 35.0), (0, 6, 30.0, 39.0), (0, 6, 30.0, 12.0), (3, 5, 32.0, 33.0), (9, 20, 30.0, 40.0), (0, 2, 30.0, 40.0),
                               (5, 5, 30.0, 40.0), (10, 4, 30.0, 40.0)]:
        assert E.stitch_clip_segment_host(seg, first, end, tl, tr) == S.clip_segment(seg, first, end, tl, tr), (first, end, tl, tr)
    assert E.stitch_clip_segment_host(seg, 0, 20, 30.0, 40.0) == seg                                   # untouched inside the range
    assert E.stitch_clip_segment_host(seg, 4, 20, 33.0, 40.0) == (4, 9, 33.0, 36.5)                    # cut in front: the seam time
    assert E.stitch_clip_segment_host(seg, 4, 20, 29.0, 40.0) == (4, 9, 31.0, 36.5)                    # clamped into the segment
    assert E.stitch_clip_segment_host(seg, 0, 6, 30.0, 39.0) == (2, 6, 31.0, 36.5)
    assert E.stitch_clip_segment_host(seg, 9, 20, 30.0, 40.0) is None and E.stitch_clip_segment_host(seg, 0, 2, 30.0, 40.0) is None
    assert S.seam_time(0, 400000, 2000000) == (25.0 + 30.0) / 2 and S.seam_time(3, 400000, 1650000) == (100.0 + 103.125) / 2


def test_stitch_applies_the_pair_rule_per_seam():
    """three windows with timestamps: the merged tokens are every window's range, and for two windows transformers' merge of
    the text tokens"""
    tw = pytest.importorskip("transformers.models.whisper.tokenization_whisper")
    ts = 50364
    a = [ts, 1, 2, 3, 4, 5, ts + 100, ts + 100, 6, 7, 8, 9, ts + 200]
    b = [ts, 6, 7, 8, 9, 10, 11, ts + 90, ts + 90, 12, 13, ts + 150]
    c = [ts, 12, 13, 14, ts + 40]
    sw, rg, merged = S.stitch([a, b], EOT)
    assert [t for t in merged if t < EOT] == tw._find_longest_common_sequence([[t for t in a if t < EOT], [t for t in b if t < EOT]])
    assert sw[0, 1:5].tolist() == [4, 4, 7, 2] and rg == [(0, 10), (3, len(b))]
    sw, rg, merged = S.stitch([a, b, c], EOT)
    assert [t for t in merged if t < EOT] == list(range(1, 15)) and rg[2] == (2, len(c))
