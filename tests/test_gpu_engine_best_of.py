"""Best-of sampling in the engine (ohw_engine_set_best_of): every rung above T = 0 samples N candidates per pending window on the
device (ohw_sample_pass_n), cuts and judges each like the device ladder's one row, and keeps the one ohw_best_of_pick_host picks.

What is checked: set_best_of(1) is the engine without the call; with N = 3 every recorded rung's kept index is the float64
restatement's pick (tests/best_of_ref.py) over ohw_seq_eval_host of the recorded candidates, the trace's pass is that candidate and
the final tokens are the kept passes'; candidate 0 of a window's first rung is the best_of = 1 device ladder's pass; in the seek
loop candidate j's generator is carried across windows and rungs, advanced by the draws each of its own cut passes used."""
import ctypes as C

import numpy as np
import pytest

import best_of_ref
from openhush_amd import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N_MAX = 220          # ohw_default_sample_params: n_text_ctx / 2 - 4


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


def _bias(n_vocab, tok, ts_b, eot_b):
    b = np.zeros(n_vocab, np.float32)
    b[tok.timestamp_begin:] = ts_b
    b[tok.eot] = eot_b
    return b


def _set_bias(E, eng, bias):
    if bias is not None:
        E.lib().ohw_state_set_logit_bias(E.lib().ohw_engine_state(eng.h), bias.ctypes.data_as(C.POINTER(C.c_float)), bias.size)


def _three_windows():
    pcm = np.concatenate([synth.synth_audio(7), synth.synth_audio(3), synth.synth_audio(11, 200000)])
    return pcm, [pcm[0:480000], pcm[480000:960000], pcm[960000:]]


def _by_win(trace):
    d = {}
    for w, T, t in trace:
        d.setdefault(w, []).append((round(T, 3), list(t)))
    return d


def _check_rungs(E, tok, eng, ends, mode=0, seeks=None, N=3, entropy_thold=None):
    """every recorded rung against the restatement and the trace; returns (rungs, rungs kept j != 0, rungs whose candidates differ)"""
    pol = E.DecodePolicy()
    E.lib().ohw_default_decode_policy(C.byref(pol))
    if entropy_thold is not None:
        pol.entropy_thold = entropy_thold
    cands = eng.last_candidates()
    trace = _by_win(eng.last_trace())
    n_nonzero = n_differ = 0
    seen = {}
    for w, T, kept, cs in cands:
        assert len(cs) == N and 0 <= kept < N
        k = seen.get(w, 0) + 1                       # the window's k-th pass of the trace (0 is the T = 0 pass)
        seen[w] = k
        evs = [E.seq_eval_host(tok, t, lp, seeks[w] if seeks else 0, ends[w], N_MAX, False, mode) for t, lp in cs]
        for (t, _), ev in zip(cs, evs):
            assert ev.n_sampled == len(t)              # recorded cut: the loop exit is the last token
        assert best_of_ref.check_pick(evs, float(pol.entropy_thold), kept), (w, T, kept, [(e.failed, e.entropy, e.avg_logprob) for e in evs])
        assert E.best_of_pick_host(evs, pol) == kept
        assert abs(trace[w][k][0] - T) < 1e-3 and trace[w][k][1] == cs[kept][0], (w, k, T)
        n_nonzero += kept != 0
        n_differ += len({tuple(t) for t, _ in cs}) > 1
    for w, passes in trace.items():
        assert len(passes) == 1 + seen.get(w, 0), w   # every rung of the trace has its record
    # the final tokens: each window's last pass, cut to what the quality record says reached the text
    q = eng.last_quality_ex()
    kept_all = []
    for w in sorted(trace):
        kept_all += trace[w][-1][1][:q[w]["n_tokens"]]
        assert abs(q[w]["temperature"] - trace[w][-1][0]) < 1e-3
    assert eng.last_tokens() == kept_all
    return len(cands), n_nonzero, n_differ


def test_best_of_1_is_the_engine_without_the_call(E, tmp_models):
    path = tmp_models("micro")
    pcm, _ = _three_windows()
    tok = E.Context.from_file(path, 0, E.OHW_DTYPE_F16).tok
    bias = _bias(51865, tok, 6.0, 27.0)
    for dev in (False, True):
        got = []
        for call in (False, True):
            eng = E.WhisperEngine.new(path, "auto", False, True, 0, E.OHW_DTYPE_F16, 3)
            eng.set_fallback_on_device(dev)
            if call:
                eng.set_best_of(1)
            _set_bias(E, eng, bias)
            res = eng.transcribe(E.AudioBuffer(pcm, 16000))
            got.append((res.text, eng.last_trace(), eng.last_quality_ex(), eng.last_tokens()))
            assert eng.last_candidates() == []
            eng.close()
        assert got[0] == got[1], dev
        assert any(q["temperature"] > 0 for q in got[0][2])          # the ladder ran


def test_best_of_3_picks_records_and_candidate_0(E, tmp_models):
    """the three-window micro case of test_device_ladder_matches_oracle_pass_by_pass_and_the_host_ladder, no bias and the
    ts 6 / eot 27 bias, N = 3.  Under the default policy the procedural model's candidates are all out (their token entropy stays
    below 2.4: it repeats itself), so every rung keeps candidate 0; the third case runs the biased input with entropy_thold 0.5,
    where candidates survive and the pick has something to choose (on MI355X: window 0 keeps j = 1 at T = 0.2 and j = 2 at 0.4)"""
    path = tmp_models("micro")
    pcm, wins = _three_windows()
    tok = E.Context.from_file(path, 0, E.OHW_DTYPE_F16).tok
    from oracle import oracle
    ends = [oracle.mel_frames(len(w)) for w in wins]
    tot = [0, 0, 0]
    for bias, ent in ((None, None), (_bias(51865, tok, 6.0, 27.0), None), (_bias(51865, tok, 6.0, 27.0), 0.5)):
        ref = E.WhisperEngine.new(path, "auto", False, True, 0, E.OHW_DTYPE_F16, 3)
        ref.set_fallback_on_device(True)
        if ent is not None:
            ref.set_decode_policy(entropy_thold=ent)
        _set_bias(E, ref, bias)
        ref.transcribe(E.AudioBuffer(pcm, 16000))
        ref_trace = _by_win(ref.last_trace())
        ref.close()
        eng = E.WhisperEngine.new(path, "auto", False, True, 0, E.OHW_DTYPE_F16, 9)      # 9 rows: three windows of three candidates
        eng.set_best_of(3)
        if ent is not None:
            eng.set_decode_policy(entropy_thold=ent)
        _set_bias(E, eng, bias)
        res = eng.transcribe(E.AudioBuffer(pcm, 16000))
        n, nz, nd = _check_rungs(E, tok, eng, ends, entropy_thold=ent)
        print(f"best_of 3, bias={'yes' if bias is not None else 'no'}, entropy_thold={ent}: {n} rungs, kept j != 0 in {nz}, candidates differ in {nd}; "
              f"temperatures kept {[round(q['temperature'], 1) for q in eng.last_quality_ex()]}")
        tot = [a + b for a, b in zip(tot, (n, nz, nd))]
        # candidate 0 of each window's first rung is the best_of = 1 device ladder's pass of that rung (its margin: one window may
        # differ - the group path's cross-attention kernel is another one, and a draw may lie at an interval edge)
        first = {}
        for w, T, kept, cs in eng.last_candidates():
            first.setdefault(w, (T, cs[0][0]))
        assert sorted(first) == sorted(w for w in ref_trace if len(ref_trace[w]) > 1)
        differ = [w for w, (T, t) in first.items() if (round(T, 3), t) != ref_trace[w][1]]
        assert len(differ) <= 1, differ
        again = eng.transcribe(E.AudioBuffer(pcm, 16000))
        assert again.text == res.text
        eng.close()
    # the inputs exercise the feature
    assert tot[0] >= 6 and tot[1] >= 1 and tot[2] >= 1, tot


def test_seek_loop_carries_one_generator_per_candidate(E, oracle, tmp_models):
    """OHW_WINDOW_SEEK, N = 3: candidate j draws from ONE std::mt19937(j) for the whole call.  Replay: HostRng(j) and the oracle's
    MT19937(j) walk the recorded candidates in the order they ran, each advanced by the tokens of its own cut pass; before every
    pass both stand at the same draw, and the oracle forced along the candidate's tokens with that generator picks the same token
    on at least 98 % of the steps (a generator one draw off gives unrelated picks) under test_gpu_policy's per-step rule"""
    from test_gpu_policy import TOL
    from test_rng_draws_cpu import _mt_canonical
    path = tmp_models("micro")
    om = oracle.Model.load(path)
    tok = E.Context.from_file(path, 0, E.OHW_DTYPE_F16).tok
    bias = _bias(om.n_vocab, tok, 8.0, 26.0)
    pcm = np.concatenate([synth.synth_audio(41), 0.1 * synth.synth_audio(42, 200000)]).astype(np.float32)
    N = 3
    eng = E.WhisperEngine.new(path, "en", False, True, 0, E.OHW_DTYPE_F16, N)
    eng.set_window_mode(E.OHW_WINDOW_SEEK)
    eng.set_best_of(N)
    _set_bias(E, eng, bias)
    eng.transcribe(E.AudioBuffer(pcm, 16000))
    q = eng.last_quality_ex()
    seek_end = oracle.mel_frames(len(pcm))
    seeks, seek = [], 0
    for x in q:
        seeks.append(seek)
        seek += x["seek_delta"] if x["seek_delta"] > 0 else 3000
    assert len(q) >= 2
    n, nz, nd = _check_rungs(E, tok, eng, [seek_end] * len(q), mode=1, seeks=seeks, N=N)
    cands = eng.last_candidates()
    assert len({w for w, _, _, _ in cands}) >= 2, "the case must fall back in two windows to carry a generator across them"
    rec_max = om.recording_max(pcm)
    host = [E.HostRng(j) for j in range(N)]
    orng = [oracle.MT19937(j) for j in range(N)]
    op = om.default_params(); op.n_max = N_MAX
    states = {}
    n_steps = n_same = 0
    for w, T, kept, cs in cands:                    # window by window, a window's rungs in order: the order the seek loop ran them
        if w not in states:
            s = oracle.State(om)
            s.set_encoder_output(om.encode(om.log_mel_seek(pcm, seeks[w], rec_max)))
            states[w] = s
        for j, (toks, _) in enumerate(cs):
            peek = type(orng[j]).from_buffer_copy(orng[j])
            assert host[j].uniforms(1)[0] == _mt_canonical(peek), (w, T, j)
            r = states[w].decode_pass(op, bias, T, orng[j], toks)
            host[j].discard_draws(len(toks))          # n_sampled_j: the candidate's own cut pass
            for i, t in enumerate(toks):
                n_steps += 1
                if r["choice"][i] == t:
                    n_same += 1
                else:
                    assert r["gaps"][i] < 0.02 or r["margins"][i] < 2 * TOL / T, (w, T, j, i, float(r["gaps"][i]), float(r["margins"][i]))
    print(f"seek loop, best_of {N}: {len(q)} windows, {n} rungs, kept j != 0 in {nz}, {n_same} / {n_steps} steps identical")
    assert n_same >= 0.98 * n_steps
    eng.close()


def test_beam_at_t0_with_best_of_on_the_rungs(E, tmp_models):
    """set_beam_size(2) + set_best_of(3), max_batch 6: batches of 6 // 3 = 2 windows, T = 0 by beam search, the rungs by best-of"""
    path = tmp_models("micro")
    pcm, wins = _three_windows()
    tok = E.Context.from_file(path, 0, E.OHW_DTYPE_F16).tok
    from oracle import oracle
    ends = [oracle.mel_frames(len(w)) for w in wins]
    assert E.batch_windows_host(6, 2, 3) == 2
    eng = E.WhisperEngine.new(path, "auto", False, True, 0, E.OHW_DTYPE_F16, 6)
    eng.set_beam_size(2)
    eng.set_best_of(3)
    _set_bias(E, eng, _bias(51865, tok, 6.0, 27.0))
    res = eng.transcribe(E.AudioBuffer(pcm, 16000))
    n, nz, nd = _check_rungs(E, tok, eng, ends)
    trace = _by_win(eng.last_trace())
    assert sorted(trace) == [0, 1, 2] and all(p[0][0] == 0.0 for p in trace.values())
    assert n >= 1 and nd >= 1
    # the T = 0 passes are the beam engine's (best_of does not touch them); two windows per batch on both sides
    beam = E.WhisperEngine.new(path, "auto", False, True, 0, E.OHW_DTYPE_F16, 4)
    beam.set_beam_size(2)
    _set_bias(E, beam, _bias(51865, tok, 6.0, 27.0))
    beam.transcribe(E.AudioBuffer(pcm, 16000))
    bt = _by_win(beam.last_trace())
    assert [trace[w][0] for w in range(3)] == [bt[w][0] for w in range(3)]
    beam.close()
    assert eng.transcribe(E.AudioBuffer(pcm, 16000)).text == res.text
    eng.close()


def test_setter_errors(E, tmp_models):
    path = tmp_models("micro")
    eng = E.WhisperEngine.new(path, "auto", False, True, 0, E.OHW_DTYPE_F16, 3)

    def refused(f, *a):
        with pytest.raises(E.WhisperError) as ex:
            f(*a)
        assert ex.value.code == E.OHW_E_INVALID_ARG
    for bad in (0, 6, -1, 4):                         # 4 > max_batch
        refused(eng.set_best_of, bad)
    eng.set_force_len(5)
    refused(eng.set_best_of, 2)                       # the setter that comes second
    eng.set_best_of(1)                                # off is always allowed
    eng.set_force_len(0)
    eng.set_best_of(3)
    refused(eng.set_force_len, 5)
    eng.set_best_of(1)
    eng.set_force_len(5)
    eng.close()


def test_pool_with_one_device_twice_equals_one_engine(E, tmp_models):
    """ohw_pool_set_best_of: device 0 listed twice gives the single engine's tokens.  max_batch 3 with best_of 3 is one window per
    batch on both sides and more than one batch per engine: all run the batch-invariant kernel variants"""
    path = tmp_models("micro")
    pcm = np.concatenate([synth.synth_audio(70 + w) for w in range(3)] + [synth.synth_audio(75, 90000)])
    eng = E.WhisperEngine.new(path, "auto", False, True, 0, E.OHW_DTYPE_F16, 3)
    eng.set_schedule(E.OHW_SCHEDULE_SEQUENTIAL)
    eng.set_best_of(3)
    ref = eng.transcribe(E.AudioBuffer(pcm, 16000))
    ref_tokens, ref_temps = eng.last_tokens(), [round(x["temperature"], 3) for x in eng.last_quality_ex()]
    assert len(eng.last_candidates()) >= 1 and any(t > 0 for t in ref_temps)
    eng.close()
    pool = E.EnginePool(path, "auto", False, [0, 0], E.OHW_DTYPE_F16, 3)
    pool.set_schedule(E.OHW_SCHEDULE_SEQUENTIAL)
    pool.set_best_of(3)
    res = pool.transcribe(E.AudioBuffer(pcm, 16000))
    assert res.text == ref.text and pool.last_tokens() == ref_tokens
    with pytest.raises(E.WhisperError):
        pool.set_best_of(4)
    pool.close()
