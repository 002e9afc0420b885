"""ohw_seek_sched (host only): the bookkeeping of many seek loops run side by side - which recordings run a window in each
round, in which slot, at which seek, and which must be uploaded.  Compared with a few lines of Python that restate the rule of
include/ohw.h, and with the single recording's loop (`seek += delta > 0 ? delta : 3000` while a second of audio is left).  No GPU.
"""
import pytest

SR = 16000
# 0.75 s (never live), exactly one window, 75 s twice (equal lengths), 31 s, 12 s, 120 s, 1.02 s (one short window)
LENS = [12000, 480000, 1200000, 1200000, 496000, 192000, 1920000, 16320]
# scripted seek_delta per recording, cycled: 0 (no timestamp: 3000), values under 3000, 3000 itself
DELTAS = [[3000], [0], [2800, 0, 1500, 2999], [1000, 100, 2400], [0, 1234], [700, 0], [2900, 50, 0, 2000, 1], [0]]


@pytest.fixture(scope="module")
def E():
    from openhush_amd import engine
    engine.lib()
    return engine


def mel_frames(n):
    return 1 + (n - 200) // 160


def step(d):
    return d if d > 0 else 3000


def single_loop_seeks(n, deltas):
    """the seeks of ohw_engine_transcribe's OHW_WINDOW_SEEK loop on one recording"""
    end, seek, out, k = mel_frames(n), 0, [], 0
    while end >= 100 and seek + 100 < end:
        out.append(seek)
        seek += step(deltas[k % len(deltas)])
        k += 1
    return out


def model_rounds(lens, deltas, max_batch):
    """the rule restated: [(rec, slot, seek, fresh)] per round"""
    end = [mel_frames(n) for n in lens]
    seek = [0] * len(lens)
    used = [0] * len(lens)
    live = lambda r: end[r] >= 100 and seek[r] + 100 < end[r]
    waiting = sorted([r for r in range(len(lens)) if live(r)], key=lambda r: -lens[r])      # stable: ties in submission order
    slots, fresh, rounds = [None] * max_batch, [0] * max_batch, []
    while True:
        for k in range(max_batch):
            if slots[k] is None and waiting:
                slots[k], fresh[k] = waiting.pop(0), 1
        rnd = [(slots[k], k, seek[slots[k]], fresh[k]) for k in range(max_batch) if slots[k] is not None]
        if not rnd:
            return rounds
        rounds.append(rnd)
        fresh = [0] * max_batch
        for r, k, _, _ in rnd:
            seek[r] += step(deltas[r][used[r] % len(deltas[r])])
            used[r] += 1
            if not live(r):
                slots[k] = None


def drive(E, lens, deltas, max_batch):
    s = E.SeekSched(lens, max_batch)
    used, rounds = [0] * len(lens), []
    while True:
        rnd = s.round()
        if not rnd:
            break
        rounds.append(rnd)
        assert len(rounds) < 1000, "the scheduler does not terminate"
        for b, (r, _, _, _) in enumerate(rnd):
            s.advance(b, deltas[r][used[r] % len(deltas[r])])
            used[r] += 1
    assert s.round() == []                # done stays done
    s.close()
    return rounds


@pytest.mark.parametrize("max_batch", [1, 2, 3, 8])
def test_rounds_follow_the_rule(E, max_batch):
    got = drive(E, LENS, DELTAS, max_batch)
    assert got == model_rounds(LENS, DELTAS, max_batch)


@pytest.mark.parametrize("max_batch", [1, 2, 3, 8])
def test_every_recording_sees_the_seeks_of_its_own_loop(E, max_batch):
    got = drive(E, LENS, DELTAS, max_batch)
    for r, n in enumerate(LENS):
        seeks = [sk for rnd in got for (rr, _, sk, _) in rnd if rr == r]
        assert seeks == single_loop_seeks(n, DELTAS[r]), r
    assert single_loop_seeks(LENS[0], DELTAS[0]) == []                   # under 1 s: no window at all
    assert single_loop_seeks(LENS[1], DELTAS[1]) == [0]                  # exactly one window
    assert len(single_loop_seeks(LENS[2], DELTAS[2])) != len(single_loop_seeks(LENS[3], DELTAS[3]))


def test_slot_order_fresh_flags_and_refill(E):
    got = drive(E, LENS, DELTAS, 2)
    # longest first, equal lengths in submission order: 120 s, then recording 2 before recording 3
    assert [(r, k, f) for r, k, _, f in got[0]] == [(6, 0, 1), (2, 1, 1)]
    order = []
    for rnd in got:
        assert [k for _, k, _, _ in rnd] == sorted(k for _, k, _, _ in rnd)          # slot order, a slot once
        assert len({k for _, k, _, _ in rnd}) == len(rnd) <= 2
        for r, k, sk, f in rnd:
            assert f == (1 if r not in order else 0)                                 # fresh exactly once, on taking the slot
            assert (sk == 0) == bool(f)
            if f:
                order.append(r)
    assert order == [6, 2, 3, 4, 1, 5, 7]                                            # recording 0 never takes a slot
    # a recording that ends frees its slot and the next waiting one takes it in the following round
    for i in range(len(got) - 1):
        here, there = {k: r for r, k, _, _ in got[i]}, {k: (r, f) for r, k, _, f in got[i + 1]}
        for k, r in here.items():
            if k in there and there[k][0] != r:
                assert there[k][1] == 1                                               # the newcomer is uploaded
                assert all(r != rr for rnd in got[i + 1:] for rr, _, _, _ in rnd)     # the one that ended never returns
    refills = [i for i in range(len(got) - 1) for r, k, _, _ in got[i]
               if any(k2 == k and r2 != r for r2, k2, _, _ in got[i + 1])]
    assert len(refills) == 5                                                         # 7 live recordings through 2 slots


def test_equal_lengths_and_only_short_recordings(E):
    got = drive(E, [480000] * 3, [[0]] * 3, 2)
    assert got == [[(0, 0, 0, 1), (1, 1, 0, 1)], [(2, 0, 0, 1)]]
    s = E.SeekSched([12000, 1600], 2)
    assert s.round() == []


def test_bad_arguments(E):
    with pytest.raises(E.WhisperError):
        E.SeekSched([], 2)
    with pytest.raises(E.WhisperError):
        E.SeekSched([480000], 0)
    with pytest.raises(E.WhisperError):
        E.SeekSched([-1], 1)
    s = E.SeekSched([480000, 480000], 2)
    with pytest.raises(E.WhisperError):
        s.advance(0, 3000)                        # no round yet
    assert len(s.round()) == 2
    s.advance(1, 0)
    with pytest.raises(E.WhisperError):
        s.advance(1, 0)                           # once per entry and round
    with pytest.raises(E.WhisperError):
        s.advance(2, 0)
