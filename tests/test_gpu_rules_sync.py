"""The four logit rules of a state (logit bias, hot phrases, repetition rule, command list) have one owner, LogitRules, and an
engine has one way of delivering them: its setters act on its own state, and the sync at the start of a transcribe makes every
other state the schedule decodes on equal to it.  Micro model (f16), force_len 12, temperature_inc 0.

Delivered late: the lane states exist before anything is set; then all four rules are set at once, two are changed and the
bias cleared, then everything is cleared.  At every stage the lanes must decode what a fresh SEQUENTIAL engine decodes that had
the settings from the start.
  The values are the existing engine tests' (hot phrases [[8911, 20198], [20198]] at boost 8, repetition (1.3, 3), the list of
  test_gpu_engine_commands.py), the list soft (penalty 6) so that the other rules still decide between listed and unlisted
  tokens, and a bias that bans 8911, which the boost would otherwise bring into every window.  Each stage's tokens must differ
  from the stages before and from the plain run, and the ban must show: the test asserts both.  Measured on the SEQUENTIAL
  engine when the values were chosen: leaving out any one of the four changes the first stage's tokens (a ban of 47018, the
  plain model's favourite, would not: the boost already keeps it out); in the second stage the boost decides alone.
A debug entry leaves the state alone: the three ohw_dbg_* rule entries run on tables of their own, also when they refuse.
"""
import ctypes as C

import numpy as np
import pytest

import command_ref as CR
import phrase_ref as PR
import repeat_ref as RR
from openhush_amd import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EOT = 50257
PHRASES, BOOST = [[8911, 20198], [20198]], 8.0
REPEAT = (1.3, 3)
LIST = [[47018, 17019], [47018, 17019, 20198], [8911], [11308, 8911, 47018], [17019, 17019, 17019], [20198, 11308], [47018, 17019]]
PENALTY = 6.0
BANNED = 8911


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from openhush_amd import engine
    engine.lib()
    return engine


def _set_bias(E, eng, bias):
    """on the engine's own state, as a caller of the C ABI does it"""
    state = E.lib().ohw_engine_state(eng.h)
    if bias is None:
        rc = E.lib().ohw_state_set_logit_bias(state, C.cast(None, C.POINTER(C.c_float)), 0)
    else:
        rc = E.lib().ohw_state_set_logit_bias(state, bias.ctypes.data_as(C.POINTER(C.c_float)), bias.size)
    assert rc == 0


def test_all_four_rules_delivered_late_to_lane_states(E, tmp_models):
    path = tmp_models("micro")
    pcm = np.concatenate([synth.synth_audio(40 + w) for w in range(3)])[:16000 * 70]
    bias = np.zeros(E.Context.from_file(path, 0, E.OHW_DTYPE_F16).hp.n_vocab, np.float32)
    bias[BANNED] = -np.inf

    def engine(schedule):
        eng = E.WhisperEngine.new(path, "en", False, True, 0, E.OHW_DTYPE_F16, 1)
        eng.set_decode_policy(temperature_inc=0.0)
        E.lib().ohw_engine_set_force_len(eng.h, 12)
        eng.set_schedule(schedule, lanes=2, merge=1)
        return eng

    def run(eng):
        eng.transcribe(E.AudioBuffer(pcm.copy(), 16000))
        return eng.last_tokens(), eng.last_commands()

    def stage_all(eng):
        _set_bias(E, eng, bias)
        eng.set_hot_phrases(PHRASES, BOOST)
        eng.set_repetition(*REPEAT)
        eng.set_commands(LIST, PENALTY)

    def stage_changed(eng):
        _set_bias(E, eng, None)
        eng.set_hot_phrases(PHRASES, 3.0)
        eng.set_repetition()

    def stage_cleared(eng):
        eng.set_hot_phrases(None)
        eng.set_commands(None)

    lanes, seq = engine(E.OHW_SCHEDULE_LANES), engine(E.OHW_SCHEDULE_SEQUENTIAL)
    try:
        plain, none = run(lanes)                        # no rule set: the lane states exist from here on
        assert len(plain) >= 36 and none == []
        seen = [plain]
        for stage in (stage_all, stage_changed):
            stage(lanes)
            stage(seq)
            got, want = run(lanes), run(seq)
            print(stage.__name__, want)
            assert got == want, stage.__name__
            assert len(want[1]) == 3 and all(want[0] != s for s in seen), stage.__name__     # the rules bite, and the change does
            seen.append(want[0])
        assert BANNED not in seen[1] and BANNED in seen[2]                         # the bias reached the lanes, and its clearing did
        stage_cleared(lanes)
        stage_cleared(seq)
        assert run(lanes) == (plain, []) and run(seq) == (plain, [])
    finally:
        lanes.close()
        seq.close()


def test_a_debug_entry_leaves_the_states_rules_alone(E, tmp_models):
    ctx = E.Context.from_file(tmp_models("micro"), 0, E.OHW_DTYPE_F16)
    st = E.State(ctx, 2)
    st.mel(np.stack([synth.synth_audio(s) for s in (11, 5)]), None, E.OHW_MEL_REFLECT, want=False)
    st.encode(2)
    st.set_phrase_table(PHRASES, BOOST)
    st.set_repeat_rule(*REPEAT)
    st.set_command_table(LIST, PENALTY)
    p = ctx.default_params(); p.n_max = 12; p.force_len = 12
    plain_st = E.State(ctx, 2)
    plain_st.mel(np.stack([synth.synth_audio(s) for s in (11, 5)]), None, E.OHW_MEL_REFLECT, want=False)
    plain_st.encode(2)
    plain = plain_st.greedy_ex(2, p)

    def snapshot():
        r = st.greedy_ex(2, p)
        return ([w["tokens"] for w in r], [np.asarray(w["logprobs"], np.float32).tobytes() for w in r], st.command_list_logprob(2).tobytes(),
                st.phrase_count(), st.command_count(), st.repeat_rule())
    before, captures = snapshot(), st.counter("step_captures")
    assert before[0] != [w["tokens"] for w in plain]                           # the state's rules are in the decode
    assert before[3:] == (2, len(LIST), (pytest.approx(1.3), 3))

    # 2 rows of 64 columns, other tables and values than the state's
    rng = np.random.default_rng(7)
    logits = rng.standard_normal((2, 64)).astype(np.float32)
    hist = np.asarray([[1, 2, 1, 0, 0, 0, 0, 0], [3, 1, 0, 0, 0, 0, 0, 0]], np.int32)
    n_cur, done, eot = [3, 2], [0, 0], 60
    small, table_boosts = [[1, 2], [3]], [2.0, 1.0]

    boosted = st.dbg_phrase_boost(logits, 64, hist, n_cur, done, E.phrase_table_build_host(small, table_boosts, eot))
    ruled = st.dbg_repeat_rule(logits, 64, hist, n_cur, done, 1.5, 2, eot)
    held, lp = st.dbg_command_rule(logits, 64, hist, [0, 1], done, E.command_table_build_host(small, eot), 3.0, eot)
    for r in range(2):                                                         # they did run, and on the caller's tables and values
        assert PR.same_words(boosted[r], PR.boost(PR.build(small, table_boosts), hist[r], n_cur[r], logits[r])), r
        assert RR.same_words(ruled[r], RR.rule(1.5, 2, hist[r], n_cur[r], logits[r], eot=eot)), r
        assert CR.same_words(held[r], CR.rule(small, 3.0, hist[r], r, logits[r], eot=eot)[0]), r
        assert not any(np.array_equal(x[r], logits[r]) for x in (boosted, ruled, held)), r
    want_lp = CR.rule(small, 3.0, hist[0], 0, logits[0], eot=eot)[1]             # row 1's history holds a text token: nothing written
    assert abs(lp[0] - want_lp) <= CR.lp_tol(eot, float(np.abs(logits).max())) and lp[1] == np.float32(-12345.0)
    # refusals: by the values ahead of everything, and by the table's check behind the upload's first step
    with pytest.raises(E.WhisperError):
        st.dbg_repeat_rule(logits, 64, hist, n_cur, done, 0.001, 2, eot)
    with pytest.raises(E.WhisperError):
        st.dbg_phrase_boost(logits[:, :2], 2, hist, n_cur, done, E.phrase_table_build_host([[1, 2], [3]], [2.0, 1.0], eot))
    with pytest.raises(E.WhisperError):
        st.dbg_command_rule(logits, 64, hist, [0, 9], done, E.command_table_build_host([[1, 2], [3]], eot), 3.0, eot)

    assert snapshot() == before
    assert st.counter("step_captures") == captures
