"""ohw_batch_plan (host only): how ohw_engine_transcribe_batch orders recordings, which context each one gets under the
engine's audio-context setting, and the envelope of every batch.  No GPU.
"""
import pytest

LENS = [17600, 80000, 480000, 48000, 1600]        # 1.1 s, 5 s, 30 s, 3 s, 0.1 s
MAX_BATCH = 2


@pytest.fixture(scope="module")
def E():
    from openhush_amd import engine
    engine.lib()
    return engine


def _batches(order, max_batch):
    return [order[i:i + max_batch] for i in range(0, len(order), max_batch)]


def test_auto_orders_longest_first_and_takes_each_recordings_own_context(E):
    order, ctx, env = E.batch_plan(LENS, MAX_BATCH, "auto")
    assert order == [2, 1, 3, 0, 4]
    assert [LENS[i] for i in order] == sorted(LENS, reverse=True)
    assert ctx == [int(E.lib().ohw_audio_ctx_for(n)) for n in LENS] == [E.audio_ctx_for(n) for n in LENS]
    assert ctx == [128, 320, 1500, 192, 64]
    assert len(env) == 3
    for e, b in zip(env, _batches(order, MAX_BATCH)):
        assert e == max(ctx[i] for i in b)
    assert env == [1500, 192, 64]


def test_equal_lengths_keep_submission_order(E):
    order, _, env = E.batch_plan([48000, 80000, 48000, 80000], 3, "auto")
    assert order == [1, 3, 0, 2] and env == [320, 192]


def test_setting_zero_is_the_full_context_everywhere(E):
    order, ctx, env = E.batch_plan(LENS, MAX_BATCH, 0)
    assert order == [2, 1, 3, 0, 4] and ctx == [1500] * 5 and env == [1500] * 3


def test_a_fixed_context_holds_for_all_or_refuses_by_index(E):
    order, ctx, env = E.batch_plan(LENS, MAX_BATCH, 1500)
    assert ctx == [1500] * 5 and env == [1500] * 3
    order, ctx, env = E.batch_plan([17600, 1600, 40960], MAX_BATCH, 128)
    assert order == [2, 0, 1] and ctx == [128] * 3 and env == [128, 128]
    with pytest.raises(E.WhisperError) as ex:
        E.batch_plan(LENS, MAX_BATCH, 128)             # 80000 > 128 * 320 = 40960: recording 1 is the first that does not fit
    assert ex.value.code == E.OHW_E_INVALID_ARG and "recording 1" in str(ex.value) and "128" in str(ex.value)


def test_more_than_one_window_is_refused_by_index(E):
    for setting in (0, "auto", 1500):
        with pytest.raises(E.WhisperError) as ex:
            E.batch_plan([17600, 80000, 480001], MAX_BATCH, setting)
        assert ex.value.code == E.OHW_E_INVALID_ARG and "recording 2" in str(ex.value)


def test_bad_arguments(E):
    L = E.lib()
    assert L.ohw_batch_plan(None, 1, 1, 0, None, None, None) == E.OHW_E_INVALID_ARG
    for setting in (-2, 1501):
        with pytest.raises((E.WhisperError, ValueError)):
            E.batch_plan(LENS, MAX_BATCH, setting)
    with pytest.raises(E.WhisperError):
        E.batch_plan(LENS, 0, 0)
