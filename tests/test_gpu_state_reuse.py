"""What one ohw_state carries from a call into the next: every decode mode of tests/state_modes.py after every other, on one
state, must give the bits it gives on a state that never ran anything else.  Micro model, both dtypes, max_batch 15.

No tolerance appears here.  Every comparison is word equality against the same build's result on a fresh state; that those
fresh results are right is pinned by the oracle and kernel tests.  This file adds only the claim that history does not matter:
arrival tickets are re-armed, double buffers and slot tables are rebuilt, per-window tables are cleared by their setters, and a
graph key names everything a captured launch bakes in ("What a state carries between calls")."""
import numpy as np
import pytest

import state_modes as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NAMES = list(M.MODES)
DTYPES = [0, 1]
# the two modes whose walk cannot capture a key twice: logits3 captures nothing (ohw_decode replays no graph), and bestof3 is
# the only mode in the group cache, which holds 4 keys.  Every other mode's key is evicted by the walk's other keys (first in,
# first out: 12 modes share the step cache of 8, 5 the beam cache of 4) and captured again when the mode returns
NEVER_EVICTED = ("logits3", "bestof3")


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from openhush_amd import engine
    engine.lib()
    return engine


@pytest.fixture(scope="module")
def ctxs(E, tmp_models):
    return {dt: E.Context.from_file(tmp_models("micro"), 0, dt) for dt in DTYPES}


def _run(E, ctx, st, fn, name):
    """one mode on one state; after a device error nothing more is launched"""
    try:
        return fn(E, ctx, st)
    except E.WhisperError as e:
        if e.code != E.OHW_E_INVALID_ARG:
            pytest.exit(f"mode {name}: the device reported an error ({e}): nothing more is launched", 3)
        raise


_FRESH = {}          # (mode, dt) -> (its result on a fresh state, the graph captures it made there)


def _fresh(E, ctxs, name, dt):
    if (name, dt) not in _FRESH:
        st = E.State(ctxs[dt], M.MAX_BATCH)
        res = _run(E, ctxs[dt], st, M.MODES[name], name)
        _FRESH[(name, dt)] = (res, st.counter("step_captures") + st.counter("beam_captures"))
        st.close()
    return _FRESH[(name, dt)]


def _describe(failures):
    return "; ".join(f"{name} after {prev}: {keys[:4]}{' ...' if len(keys) > 4 else ''} first differing index {at}"
                     for prev, name, keys, at in failures)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_modes_repeat_on_fresh_states(E, ctxs, name, dt):
    """run-to-run determinism (the ticket merges run in slice order): the mode on two fresh states gives the same words"""
    first, _ = _fresh(E, ctxs, name, dt)
    assert first and any(len(v) > 0 for v in first.values())
    st =E.State(ctxs[dt], M.MAX_BATCH)
    second = _run(E, ctxs[dt], st, M.MODES[name], name)
    st.close()
    bad = M.same(second, first)
    assert not bad, (name, dt, bad, M.first_difference(second, first, bad[0]))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("a", NAMES)
def test_mode_after_mode(E, ctxs, a, dt):
    """one state walks a, b0, a, b1, ..., a: every (a, b) and (b, a) is a pair of neighbouring calls, and every result equals
    the mode's result on a fresh state.  The walk holds more graph keys than the step cache (8) keeps - and, from a beam mode,
    more than the beam cache (4) - so mode a's iteration is evicted and captured again on the way: more captures than keys"""
    ctx = ctxs[dt]
    fresh = {b: _fresh(E, ctxs, b, dt)[0] for b in NAMES}
    keys = sum(_fresh(E, ctxs, b, dt)[1] for b in NAMES)        # an upper bound of the distinct keys: every mode's own captures
    st = E.State(ctx, M.MAX_BATCH)
    failures = M.walk(lambda b: _run(E, ctx, st, M.MODES[b], b), M.schedule(a, NAMES), fresh)
    captures = st.counter("step_captures") + st.counter("beam_captures")
    st.close()
    assert not failures, (a, dt, _describe(failures))
    if a in NEVER_EVICTED:
        # every other mode runs once in this walk, so each of its keys is captured once, and mode a's own are never evicted
        assert captures == keys, (a, dt, captures, keys)
    else:
        assert captures > keys, (a, dt, captures, keys)          # at least one key was captured more than once


@pytest.mark.parametrize("dt", DTYPES)
def test_the_walk_sees_a_leak(E, ctxs, dt):
    """the harness itself: with a greedy_bias that leaves its bias on the state as mode a, the walk reports the modes that
    decode without a bias of their own as differing after it"""
    ctx = ctxs[dt]
    names = ["greedy3", "greedy1", "beam2", "invariant"]
    fresh = {b: _fresh(E, ctxs, b, dt)[0] for b in names}
    fresh["leaky"] = _fresh(E, ctxs, "greedy_bias", dt)[0]       # the leaky copy itself computes what greedy_bias computes
    modes = dict(M.MODES, leaky=M.leaky_greedy_bias)
    st = E.State(ctx, M.MAX_BATCH)
    failures = M.walk(lambda b: _run(E, ctx, st, modes[b], b), M.schedule("leaky", names), fresh)
    st.close()
    seen = {(prev, name) for prev, name, _, _ in failures}
    # beam2 sets the bias itself and clears it: it does not differ, and what follows it runs clean until the leak returns
    assert ("leaky", "greedy3") in seen and ("leaky", "greedy1") in seen and ("leaky", "invariant") in seen, _describe(failures)
    assert ("leaky", "beam2") not in seen and not any(name == "leaky" for _, name, _, _ in failures), _describe(failures)
    for prev, name, keys, at in failures:
        assert prev == "leaky" and any(k.endswith(".logprobs") for k in keys) and at >= 0, (prev, name, keys, at)


def test_modes_on_a_small_state(E, ctxs):
    """logits3, beam2 and bestof3 need 3, 6 and 6 decoder rows: on a state of 6 they give the words they give on a state of 15
    (no stride of a row, slot or history buffer may depend on max_batch in a way a result can see)"""
    for dt in DTYPES:
        for name in ("logits3", "beam2", "bestof3"):
            st = E.State(ctxs[dt], 6)
            got = _run(E, ctxs[dt], st, M.MODES[name], name)
            st.close()
            want = _fresh(E, ctxs, name, dt)[0]
            bad = M.same(got, want)
            assert not bad, (name, dt, bad, M.first_difference(got, want, bad[0]))
