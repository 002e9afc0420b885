"""Recording slots (ohw_recording_set_slot / ohw_mel_seek_slots): a state holds one recording per slot and cuts window b from
the spectrogram of the recording in slots[b], clamped with that recording's own maximum.

The statement is equality of bits with the single-recording path (ohw_recording_set / ohw_mel_seek of that recording at that
seek on a second state): the DFT arithmetic is the same and the atomic maximum is order-independent.  The oracle's
restatement of whisper.cpp's whole-input front end bounds both (2e-4, the tolerance of test_gpu_parity.py).  Micro model, f16.
"""
import numpy as np
import pytest

from openhush_amd import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from openhush_amd import engine
    assert hasattr(engine.lib(), "ohw_recording_set_slot") and hasattr(engine.lib(), "ohw_mel_seek_slots")
    return engine


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o
    return o


@pytest.fixture(scope="module")
def recs():
    """quiet-then-loud (test_mel_seek_windows_of_the_recording_wide_spectrogram's), 300 000 samples, a loud 70 s"""
    a = np.concatenate([0.05 * synth.synth_audio(21), synth.synth_audio(22), 0.2 * synth.synth_audio(23, 150000)]).astype(np.float32)
    b = synth.synth_audio(7, 300000).astype(np.float32)
    c = (30.0 * np.concatenate([synth.synth_audio(51), synth.synth_audio(52), synth.synth_audio(53, 160000)])).astype(np.float32)
    return [a, b, c]


# per recording: seek 0, one across a loud part, one into the zero tail (frames past the last sample)
SEEKS = [[0, 1234, 4700], [0, 700, 1900], [0, 2500, 6900]]


@pytest.fixture(scope="module")
def world(E, oracle, tmp_models, recs):
    """the context, a 3-slot state, and the single-recording path's maxima and windows from a SECOND state (computed once)"""
    path = tmp_models("micro")
    ctx = E.Context.from_file(path, 0, E.OHW_DTYPE_F16)
    om = oracle.Model.load(path)
    lone = E.State(ctx, 3)
    lone_max, lone_win = [], []
    for r, sk in zip(recs, SEEKS):
        lone_max.append(lone.recording_set(r))
        lone_win.append(lone.mel_seek(sk).copy())
    lone.close()
    st = E.State(ctx, 3)
    yield {"E": E, "ctx": ctx, "om": om, "st": st, "lone_max": lone_max, "lone_win": lone_win}
    st.close()


def test_refusals_before_any_slot_is_set(world, recs):
    E, st = world["E"], world["st"]
    with pytest.raises(E.WhisperError) as ex:
        st.mel_seek_slots([0], [0])                              # an empty slot
    assert ex.value.code == E.OHW_E_INVALID_ARG
    with pytest.raises(E.WhisperError) as ex:
        st.recording_set_slot(3, recs[1])                        # a slot >= max_batch
    assert ex.value.code == E.OHW_E_INVALID_ARG
    with pytest.raises(E.WhisperError):
        st.recording_set_slot(-1, recs[1])
    with pytest.raises(E.WhisperError) as ex:
        st.recording_set_slot(0, np.zeros(0, np.float32))        # n < 1
    assert ex.value.code == E.OHW_E_INVALID_ARG


def test_each_slot_finds_its_own_maximum(world, recs):
    st, om = world["st"], world["om"]
    got = [st.recording_set_slot(k, r) for k, r in enumerate(recs)]
    for k, r in enumerate(recs):
        assert got[k] == world["lone_max"][k], k                 # exactly ohw_recording_set's
        assert abs(got[k] - om.recording_max(r)) < 1e-4, k
    assert got[2] - got[0] > 0.5 and len(set(got)) == 3          # three different clamps: an index mix-up shows


def test_windows_equal_the_single_recording_path_bit_for_bit(world, recs):
    st, om = world["st"], world["om"]
    for k, r in enumerate(recs):
        st.recording_set_slot(k, r)
    # mixed slot lists: every slot, a permutation, a slot used twice in one call, one window alone
    calls = [([0, 1, 2], [0, 0, 0]), ([2, 0, 1], [1, 1, 1]), ([1, 1, 0], [2, 0, 2]), ([2, 2, 2], [0, 2, 1]), ([0], [1])]
    checked = set()
    for slots, which in calls:
        got = st.mel_seek_slots(slots, [SEEKS[s][w] for s, w in zip(slots, which)])
        for b, (s, w) in enumerate(zip(slots, which)):
            assert np.array_equal(got[b], world["lone_win"][s][w]), (slots, which, b)
            if (s, w) not in checked:                            # the oracle bounds every (recording, seek) once
                checked.add((s, w))
                ref = om.log_mel_seek(recs[s], SEEKS[s][w], om.recording_max(recs[s]))
                assert np.abs(got[b] - ref).max() < 2e-4, (s, w, float(np.abs(got[b] - ref).max()))
    assert len(checked) == 9
    # the encoder consumes the windows as after ohw_mel_seek
    st.mel_seek_slots([1, 0], [0, 1234], want=False)
    st.encode(2)
    assert np.isfinite(st.fetch("enc", 2)).all()


def test_needle_a_wrong_maximum_index_shows(world, recs):
    om = world["om"]
    quiet0 = world["lone_win"][0][0]                             # the quiet first window, clamped with its own recording's maximum
    wrong = om.log_mel_seek(recs[0], 0, om.recording_max(recs[2]))       # ... with the loud neighbour's
    assert np.abs(quiet0 - wrong).max() > 0.5
    st = world["st"]
    for k, r in enumerate(recs):
        st.recording_set_slot(k, r)
    assert np.array_equal(st.mel_seek_slots([2, 0], [0, 0])[1], quiet0)


def test_needle_a_shorter_recording_in_the_same_slot_sees_nothing_old(world, recs):
    st = world["st"]
    st.recording_set_slot(1, recs[2])                            # the loud 70 s recording ...
    assert np.array_equal(st.mel_seek_slots([1], [SEEKS[2][1]])[0], world["lone_win"][2][1])
    mx = st.recording_set_slot(1, recs[1])                       # ... then the 300 000-sample one
    assert mx == world["lone_max"][1]                            # not the loud one's maximum
    got = st.mel_seek_slots([1, 1], [SEEKS[1][1], SEEKS[1][2]])  # both reach past the short one's end (1875 frames)
    assert np.array_equal(got[0], world["lone_win"][1][1]) and np.array_equal(got[1], world["lone_win"][1][2])
    assert SEEKS[1][1] + 3000 > len(recs[1]) // 160 and SEEKS[1][2] > len(recs[1]) // 160


def test_refusals_with_slots_set(world, recs):
    E = world["E"]
    st2 = E.State(world["ctx"], 3)
    st2.recording_set_slot(1, recs[1])
    n_len = (len(recs[1]) + 480000) // 160
    for slots, seeks in (([0], [0]), ([1, 2], [0, 0]),           # empty slots
                         ([3], [0]), ([-1], [0]),                # slots outside the state
                         ([1], [n_len]), ([1], [-1]),            # a seek past the frames
                         ([1, 1, 1, 1], [0, 0, 0, 0])):          # batch > max_batch
        with pytest.raises(E.WhisperError) as ex:
            st2.mel_seek_slots(slots, seeks)
        assert ex.value.code == E.OHW_E_INVALID_ARG, (slots, seeks)
    assert st2.mel_seek_slots([1], [n_len - 1]).shape[0] == 1    # the last frame is inside
    st2.close()


def test_the_single_recording_keeps_its_bits_on_the_same_state(world, recs):
    st = world["st"]
    for k, r in enumerate(recs):
        st.recording_set_slot(k, r)
    for k in (2, 0):
        assert st.recording_set(recs[k]) == world["lone_max"][k]
        assert np.array_equal(st.mel_seek(SEEKS[k]), world["lone_win"][k])
        # and the slots are untouched by it
        assert np.array_equal(st.mel_seek_slots([1], [SEEKS[1][1]])[0], world["lone_win"][1][1])
