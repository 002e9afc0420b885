"""Beam search in the engine (ohw_engine_set_beam_size): the T = 0 pass of every transcribe is ohw_beam_search_ex, judged by
whisper.cpp's per-window policy, with the temperature ladder, the seek loop, the batch calls, prompts and word timestamps as
they are for the greedy pass.  micro model, f16.

How a transcribe is compared (the walk of test_gpu_policy.py, restated with a beam pass in front):
  * the traced T = 0 tokens of a window are State.beam_search_ex's winner on the same window, cut at the oracle's
    evaluate_sequence(...).n_sampled - beam search is not causal, so the loop exits are applied to the winner after the search;
  * that winner against the oracle's own beam search by test_gpu_beam.py's criterion: the oracle's exact winner, or a sequence
    that scores as well under the oracle (cumulative log-probability per token within 0.02 of its best candidate), and at
    least 70 % of the windows exact;
  * every later pass is replayed on the oracle along the engine's tokens with the same generator state, and the decisions
    (retry, kept tokens, no-speech) and the quality record must be the oracle's."""
import ctypes as C

import numpy as np
import pytest

from openhush_amd import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOL = 0.03          # f16 logits (test_gpu_policy.py)


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from openhush_amd import engine
    engine.lib()
    return engine


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o
    return o


def _bias(om, ts_b, eot_b):
    b = np.zeros(om.n_vocab, np.float32)
    b[om.tok_beg:] = ts_b
    b[om.tok_eot] = eot_b
    return b


def _set_bias(E, eng, bias):
    st = E.lib().ohw_engine_state(eng.h)
    if bias is None:
        assert E.lib().ohw_state_set_logit_bias(st, C.cast(None, C.POINTER(C.c_float)), 0) == 0
    else:
        assert E.lib().ohw_state_set_logit_bias(st, bias.ctypes.data_as(C.POINTER(C.c_float)), bias.size) == 0


def _walk_and_compare(E, oracle, om, eng, windows_pcm, bias, pol, winners=None, seeks=None, ends=None, mode=0, n_max=220, mels=None):
    """test_gpu_policy.py's _walk_and_compare with a beam pass at T = 0.  winners (or None): per window State.beam_search_ex's
    result on the same window.  -> (passes, steps of the passes at T > 0, steps where the oracle's own pick is the engine's)"""
    trace = eng.last_trace()
    qual = eng.last_quality_ex()
    op = om.default_params(); op.n_max = n_max
    by_win = {}
    for w, T, toks in trace:
        by_win.setdefault(w, []).append((T, toks))
    assert sorted(by_win) == list(range(len(windows_pcm)))
    temps = [0.0] + ([round(pol.temperature_inc * k, 6) for k in range(1, 100) if pol.temperature_inc * k < 1.0 + 1e-6] if pol.temperature_inc > 0 else [])
    n_pass = n_steps = n_same = 0
    shared_rng = oracle.MT19937(0)
    kept_all = []
    for w in sorted(by_win):
        s = oracle.State(om)
        s.set_encoder_output(om.encode(mels[w] if mels is not None else om.log_mel(windows_pcm[w], 1)))
        rng = shared_rng if mode == 1 else oracle.MT19937(0)
        seek = seeks[w] if seeks else 0
        end = ends[w] if ends else oracle.mel_frames(len(windows_pcm[w]))
        passes = by_win[w]
        first_again = False
        for k, (T, toks) in enumerate(passes):
            assert abs(T - temps[k]) < 1e-3, (w, k, T)
            r = s.decode_pass(op, bias, T, rng, toks)
            assert len(r["choice"]) >= len(toks)
            if k == 0:
                # the beam pass: not the oracle's greedy path, so no step-by-step pick.  It is the search's winner, cut
                if winners is not None:
                    g = winners[w]
                    full = g["tokens"] + ([om.tok_eot] if g["ended_by_eot"] else [])
                    rf = s.decode_pass(op, bias, 0.0, None, full)
                    cut = oracle.evaluate_sequence(om, full, rf["plogs"], seek, end, n_max, False, mode).n_sampled
                    assert toks == full[:cut], (w, toks, full, cut)
            else:
                for i, t in enumerate(toks):
                    n_steps += 1
                    if r["choice"][i] == t:
                        n_same += 1
                    else:
                        # a draw next to an interval edge, or a near-tie of the timestamp-mass rule
                        assert r["gaps"][i] < 0.02 or r["margins"][i] < 2 * TOL / T, (w, k, i, t, r["choice"][i], float(r["gaps"][i]), float(r["margins"][i]))
            ev = oracle.evaluate_sequence(om, toks, r["plogs"], seek, end, n_max, False, mode)
            assert ev.n_sampled == len(toks), (w, k, ev.n_sampled, len(toks))       # cut where whisper.cpp's loop exits
            again = oracle.pass_needs_fallback(ev, pol, r["no_speech_prob"], k == len(temps) - 1)
            if k == 0:
                first_again = oracle.pass_needs_fallback(ev, pol, r["no_speech_prob"], False)
            assert again == (k + 1 < len(passes)), (w, k, T, ev.as_dict(), r["no_speech_prob"])
            n_pass += 1
        q = qual[w]
        ns = oracle.window_is_no_speech(ev, pol, r["no_speech_prob"])
        assert q["no_speech"] == ns and q["failed"] == bool(ev.failed) and q["result_len"] == ev.result_len and q["seek_delta"] == ev.seek_delta
        assert abs(q["temperature"] - passes[-1][0]) < 1e-3 and q["would_fallback"] == first_again
        keep = 0 if ns else ev.n_keep
        assert q["n_tokens"] == keep
        kept_all += passes[-1][1][:keep]
        if ev.result_len > 0:
            assert abs(q["avg_logprob"] - ev.avg_logprob) < 2 * TOL and abs(q["entropy"] - ev.entropy) < 1e-4
    assert eng.last_tokens() == kept_all
    return n_pass, n_steps, n_same


PCM3 = None


def _three_windows():
    global PCM3
    if PCM3 is None:
        PCM3 = np.concatenate([synth.synth_audio(7), synth.synth_audio(3), synth.synth_audio(11, 200000)])
    pcm = PCM3
    return pcm, [pcm[0:480000], pcm[480000:960000], pcm[960000:]]


def test_fixed_cuts_beam_pass_ladder_and_batch_cutting(E, oracle, tmp_models):
    """Three windows, K = 5, max_batch 15 (one batch of three) and 5 (three batches of one), with and without the timestamp /
    end-of-text bias; set_beam_size(0) afterwards is the greedy engine again."""
    path = tmp_models("micro")
    om = oracle.Model.load(path)
    ctx = E.Context.from_file(path, 0, E.OHW_DTYPE_F16)
    pcm, wins = _three_windows()
    pol = oracle.default_policy()
    K = 5
    exact = total = 0
    tot_steps = tot_same = 0
    for bias in (_bias(om, 6.0, 27.0), None):
        eng = E.WhisperEngine.new(path, "auto", False, True, 0, E.OHW_DTYPE_F16, 15)
        _set_bias(E, eng, bias)
        eng.set_beam_size(K)
        res = eng.transcribe(E.AudioBuffer(pcm, 16000))
        # the same windows through the state-level search: one batch of three, 15 rows, as the engine ran them
        st = E.State(ctx, 3 * K)
        st.set_logit_bias(bias)
        stage = np.zeros((3, 480000), np.float32)
        for w, x in enumerate(wins):
            stage[w, :len(x)] = x
        mel = st.mel(stage, [len(x) for x in wins], E.OHW_MEL_ZERO_TAIL)
        st.encode(3)
        winners = st.beam_search_ex(3, K, ctx.default_params())
        st.close()
        n_pass, n_steps, n_same = _walk_and_compare(E, oracle, om, eng, wins, bias, pol, winners=winners)
        tot_steps += n_steps; tot_same += n_same
        print(f"engine beam {K}: bias={'yes' if bias is not None else 'no'}: {n_pass} passes, {n_same} / {n_steps} ladder steps identical; "
              f"temperatures kept {[round(q['temperature'], 1) for q in eng.last_quality_ex()]}")
        if bias is None:
            assert n_pass == 18 and all(abs(q["temperature"] - 1.0) < 1e-3 for q in eng.last_quality_ex())      # the whole ladder
        # the search itself against the oracle's (test_gpu_beam.py's criterion)
        op = om.default_params()
        for w in range(3):
            enc = om.encode(om.log_mel(wins[w], 1))
            assert np.abs(mel[w] - om.log_mel(wins[w], 1)).max() < 2e-4
            ref = oracle.beam_search(om, enc, op, K, bias)
            g = winners[w]
            total += 1
            if g["tokens"] == ref["tokens"]:
                exact += 1
                assert abs(g["sum_logprob"] - ref["sum_logprob"]) < 0.06 * max(1, len(g["tokens"])) ** 0.5
            else:
                s = oracle.State(om); s.set_encoder_output(enc)
                best = max(c[1] / max(1, len(c[0])) for c in ref["candidates"])
                mine = max(s.score_sequence(op, g["tokens"], e, bias) / max(1, len(g["tokens"])) for e in (True, False))
                assert mine > best - 0.02, (w, g, ref["tokens"], mine, best)
        # max_batch = 5: the same three windows go through three batches of one.  A call of several batches runs batch-invariant
        # (kernel variants no longer picked from a batch's row count), so the one batch of three it is compared with does too:
        # that is the mode in which a window's bits do not depend on its batch (without it a draw of the ladder at T = 1.0 next to
        # an interval edge may fall on the other side)
        state = E.lib().ohw_engine_state(eng.h)
        assert E.lib().ohw_state_set_batch_invariant(state, 1) == 0
        inv = eng.transcribe(E.AudioBuffer(pcm, 16000))
        tokens15, trace15 = eng.last_tokens(), eng.last_trace()
        assert [w for w, T, _ in trace15 if T == 0.0] == [0, 1, 2]
        print(f"  one batch of three, batch invariance off / on: text {'equal' if inv.text == res.text else 'differs'}")
        eng.close()
        eng5 = E.WhisperEngine.new(path, "auto", False, True, 0, E.OHW_DTYPE_F16, 5)
        _set_bias(E, eng5, bias)
        eng5.set_beam_size(K)
        r5 = eng5.transcribe(E.AudioBuffer(pcm, 16000))
        assert eng5.last_trace() == trace15
        assert r5.text == inv.text and eng5.last_tokens() == tokens15
        if bias is not None:
            # beam off again: a fresh greedy engine's result
            eng5.set_beam_size(0)
            g5 = eng5.transcribe(E.AudioBuffer(pcm, 16000))
            fresh = E.WhisperEngine.new(path, "auto", False, True, 0, E.OHW_DTYPE_F16, 5)
            _set_bias(E, fresh, bias)
            gf = fresh.transcribe(E.AudioBuffer(pcm, 16000))
            assert g5.text == gf.text and eng5.last_tokens() == fresh.last_tokens() and eng5.last_trace() == fresh.last_trace()
            assert eng5.last_trace() != trace15
            fresh.close()
        eng5.close()
    print(f"engine beam search: {exact} / {total} windows with the oracle's exact winner; ladder {tot_same} / {tot_steps} steps identical")
    assert exact >= 0.7 * total
    assert tot_same >= 0.98 * tot_steps


def test_seek_mode_walk(E, oracle, tmp_models):
    """OHW_WINDOW_SEEK with the timestamp bias: the walk with seeks taken from the quality records, one generator for the call"""
    path = tmp_models("micro")
    om = oracle.Model.load(path)
    ctx = E.Context.from_file(path, 0, E.OHW_DTYPE_F16)
    bias = _bias(om, 8.0, 26.0)
    K = 5
    pcm = np.concatenate([synth.synth_audio(41), 0.1 * synth.synth_audio(42, 200000)]).astype(np.float32)
    eng = E.WhisperEngine.new(path, "en", False, True, 0, E.OHW_DTYPE_F16, K)
    eng.set_window_mode(E.OHW_WINDOW_SEEK)
    _set_bias(E, eng, bias)
    eng.set_beam_size(K)
    pol = oracle.default_policy()
    eng.transcribe(E.AudioBuffer(pcm, 16000))
    q = eng.last_quality_ex()
    seek_end = oracle.mel_frames(len(pcm))
    seeks, wins = [], []
    seek = 0
    for x in q:
        seeks.append(seek)
        wins.append(pcm[seek * 160: seek * 160 + 480000])
        seek += x["seek_delta"] if x["seek_delta"] > 0 else 3000
    assert seek + 100 >= seek_end and len(q) >= 2
    assert any(x["seek_delta"] != 3000 for x in q)
    rec_max = om.recording_max(pcm)
    mels = [om.log_mel_seek(pcm, sk, rec_max) for sk in seeks]
    # the state-level search on each window of the recording-wide spectrogram
    st = E.State(ctx, K)
    st.set_logit_bias(bias)
    st.recording_set(pcm)
    p = ctx.default_params(); p.lang_id = E.lang_code_to_id("en")
    winners = []
    for sk in seeks:
        st.mel_seek([sk], want=False)
        st.encode(1)
        winners.append(st.beam_search_ex(1, K, p)[0])
    st.close()
    n_pass, n_steps, n_same = _walk_and_compare(E, oracle, om, eng, wins, bias, pol, winners=winners, seeks=seeks, ends=[seek_end] * len(q), mode=1, mels=mels)
    print(f"seek loop, beam {K}: {len(q)} windows, seek deltas {[x['seek_delta'] for x in q]}, {n_pass} passes, {n_same} / {n_steps} ladder steps identical")
    assert n_same >= 0.98 * n_steps
    eng.close()


QKEYS = ("result_len", "seek_delta", "failed", "no_speech", "would_fallback", "temperature", "n_tokens", "avg_logprob", "entropy", "no_speech_prob")


def _alone(E, eng, pcm, mode):
    """transcribe() of one recording with batch invariance on, as the batch calls run -> (text, tokens, quality records)"""
    state = E.lib().ohw_engine_state(eng.h)
    eng.set_window_mode(mode)
    assert E.lib().ohw_state_set_batch_invariant(state, 1) == 0
    r = eng.transcribe(E.AudioBuffer(pcm.copy(), 16000))
    out = (r.text, eng.last_tokens(), [{k: x[k] for k in QKEYS} for x in eng.last_quality_ex()])
    E.lib().ohw_state_set_batch_invariant(state, 0)
    eng.set_window_mode(E.OHW_WINDOW_FIXED)
    return out


def test_batch_calls_equal_every_recording_alone(E, oracle, tmp_models):
    """transcribe_batch and transcribe_long_batch with K = 3 on an engine of 7 rows (two windows per decode batch): recording i's
    text, tokens and quality records are transcribe()'s on it alone with the same beam size"""
    path = tmp_models("micro")
    om = oracle.Model.load(path)
    bias = _bias(om, 8.0, 26.0)
    K = 3
    eng = E.WhisperEngine.new(path, "en", False, True, 0, E.OHW_DTYPE_F16, 7)
    _set_bias(E, eng, bias)
    eng.set_beam_size(K)
    short = [synth.synth_audio(21, 240000), synth.synth_audio(22), synth.synth_audio(23, 100000)]            # 15 s, 30 s, 6.25 s
    res = eng.transcribe_batch([E.AudioBuffer(x, 16000) for x in short])
    got = [eng.batch_result(i) for i in range(3)]
    for i, x in enumerate(short):
        text, toks, qs = _alone(E, eng, x, E.OHW_WINDOW_FIXED)
        assert (res[i].text, got[i][1]) == (text, toks), i
        assert {k: got[i][2][k] for k in QKEYS} == qs[0], i
    assert any(r.text for r in res)
    long_ = [synth.synth_audio(21, 240000), np.concatenate([synth.synth_audio(41), 0.1 * synth.synth_audio(42, 200000)]).astype(np.float32),
             synth.synth_audio(23, 100000)]                                                                  # the second: 42.5 s
    res = eng.transcribe_long_batch([E.AudioBuffer(x, 16000) for x in long_])
    got = [(eng.batch_result(i), eng.long_batch_quality(i)) for i in range(3)]
    n_windows = []
    for i, x in enumerate(long_):
        text, toks, qs = _alone(E, eng, x, E.OHW_WINDOW_SEEK)
        assert (res[i].text, got[i][0][1]) == (text, toks), i
        assert [{k: y[k] for k in QKEYS} for y in got[i][1]] == qs, i
        n_windows.append(len(qs))
    assert n_windows[1] >= 2
    eng.close()


def test_prompt_and_word_timestamps(E, oracle, tmp_models):
    path = tmp_models("micro")
    om = oracle.Model.load(path)
    bias = _bias(om, 6.0, 27.0)
    pcm, wins = _three_windows()
    eng = E.WhisperEngine.new(path, "auto", False, True, 0, E.OHW_DTYPE_F16, 15)
    _set_bias(E, eng, bias)
    eng.set_beam_size(5)
    plain = eng.transcribe(E.AudioBuffer(pcm, 16000))
    plain_tokens = eng.last_tokens()
    eng.set_word_timestamps([(0, 1), (1, 3)])
    timed = eng.transcribe(E.AudioBuffer(pcm, 16000))
    assert timed.text == plain.text and eng.last_tokens() == plain_tokens
    tt = eng.last_token_times()
    assert len(tt) == sum(1 for t in plain_tokens if t < om.tok_eot) and len(tt) > 0
    for a, b in zip(tt, tt[1:]):
        assert a["t0"] <= a["t1"] and (b["window"] != a["window"] or a["t1"] <= b["t0"] + 1e-6)
    eng.set_initial_prompt(" w1 w2")
    prompted = eng.transcribe(E.AudioBuffer(pcm, 16000))
    assert len(eng.last_quality_ex()) == 3 and isinstance(prompted.text, str)
    tt = eng.last_token_times()
    for a, b in zip(tt, tt[1:]):
        assert a["t0"] <= a["t1"] and (b["window"] != a["window"] or a["t1"] <= b["t0"] + 1e-6)
    eng.set_initial_prompt(None)
    eng.set_word_timestamps(None)
    assert eng.transcribe(E.AudioBuffer(pcm, 16000)).text == plain.text
    eng.close()


def test_setter_errors_leave_the_engine_usable(E, tmp_models):
    path = tmp_models("micro")
    eng = E.WhisperEngine.new(path, "auto", False, True, 0, E.OHW_DTYPE_F16, 3)
    eng.set_decode_policy(temperature_inc=0.0)
    pcm = synth.synth_audio(5, 160000)
    base = eng.transcribe(E.AudioBuffer(pcm, 16000)).text

    def refused(f, *a):
        with pytest.raises(E.WhisperError) as ex:
            f(*a)
        assert ex.value.code == E.OHW_E_INVALID_ARG, ex.value

    refused(eng.set_beam_size, 1)
    refused(eng.set_beam_size, 6)
    refused(eng.set_beam_size, 4)            # k > max_batch
    refused(eng.set_beam_size, -1)
    assert eng.transcribe(E.AudioBuffer(pcm, 16000)).text == base
    eng.set_force_len(5)
    refused(eng.set_beam_size, 3)            # the setter that comes second
    eng.set_force_len(0)
    eng.set_beam_size(3)
    refused(eng.set_force_len, 5)
    beam = eng.transcribe(E.AudioBuffer(pcm, 16000))
    assert isinstance(beam.text, str) and len(eng.last_quality_ex()) == 1
    eng.set_beam_size(0)
    assert eng.transcribe(E.AudioBuffer(pcm, 16000)).text == base
    eng.close()


def test_pool_forwards_the_beam_size(E, tmp_models):
    path = tmp_models("micro")
    pcm = np.concatenate([synth.synth_audio(70 + w) for w in range(3)] + [synth.synth_audio(75, 90000)])      # 4 windows, short tail
    # 3 rows per engine: every decode batch is one window of three beams, on the single engine and on both engines of the pool
    eng = E.WhisperEngine.new(path, "auto", False, True, 0, E.OHW_DTYPE_F16, 3)
    eng.set_decode_policy(temperature_inc=0.0)
    eng.set_beam_size(3)
    ref = eng.transcribe(E.AudioBuffer(pcm, 16000))
    ref_tokens = eng.last_tokens()
    eng.close()
    pool = E.EnginePool(path, "auto", False, [0, 0], E.OHW_DTYPE_F16, 3)
    pool.set_decode_policy(temperature_inc=0.0)
    pool.set_beam_size(3)
    res = pool.transcribe(E.AudioBuffer(pcm, 16000))
    assert res.text == ref.text and pool.last_tokens() == ref_tokens
    with pytest.raises(E.WhisperError):
        pool.set_beam_size(7)
    pool.close()
