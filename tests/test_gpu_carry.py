"""Carried context in the engine's seek loops (ohw_engine_set_carry_context): every window of OHW_WINDOW_SEEK transcribe and of
ohw_engine_transcribe_long_batch decodes behind the tail of what the recording's earlier windows produced.  Micro model file,
f16, max_batch 2 (4 for beam 2), the timestamp / end-of-text bias and the recordings of test_gpu_long_batch.py.

The rule is restated in carry_ref.py; what the engine decoded behind is read back with last_contexts() / long_batch_contexts()
and, for the device side, replayed by hand on a state of a second context."""
import ctypes as C
import struct

import numpy as np
import pytest

import carry_ref as R
import test_gpu_long_batch as LB
from test_gpu_long_batch import E, oracle_tokens, recs  # noqa: F401 - fixtures

pytestmark = pytest.mark.gpu

N_TEXT_CTX = 448           # synth.PRESETS["micro"].n_text_ctx
CAP = N_TEXT_CTX // 2 - 1
# host ladder against device ladder: a token's log-probability is logit - logsumexp over 51865 fp32 terms, |value| < 64 under the
# bias of 26, where an fp32 ulp is 3.8e-6; two summation orders differ by a few ulps of the result, and an average of such
# values by no more: 16 ulps
FLOAT_TOL = 16 * 2.0 ** -18


def _engine(E, path, oracle_tokens, max_batch=LB.MAX_BATCH, temperature_inc=0.0, device_ladder=False):
    """test_gpu_long_batch's engine, with the batch size a parameter"""
    eng = E.WhisperEngine.new(path, "en", False, True, 0, E.OHW_DTYPE_F16, max_batch)
    if temperature_inc is not None:
        eng.set_decode_policy(temperature_inc=temperature_inc)
    eng.set_fallback_on_device(device_ladder)
    bias = _bias(oracle_tokens)
    E.lib().ohw_state_set_logit_bias(E.lib().ohw_engine_state(eng.h), bias.ctypes.data_as(C.POINTER(C.c_float)), bias.size)
    assert hasattr(E.lib(), "ohw_engine_set_carry_context") and hasattr(E.lib(), "ohw_engine_last_context")
    return eng


def _bias(oracle_tokens):
    tok_beg, tok_eot, n_vocab = oracle_tokens
    bias = np.zeros(n_vocab, np.float32)
    bias[tok_beg:] = 8.0
    bias[tok_eot] = 26.0
    return bias


def _alone(E, eng, pcm):
    out = LB._alone(E, eng, pcm)
    out["contexts"] = eng.last_contexts()
    assert len(out["contexts"]) == len(out["quality"])
    return out


def _together(E, eng, pcms):
    out = LB._together(E, eng, pcms)
    for i, o in enumerate(out):
        o["contexts"] = eng.long_batch_contexts(i)
        assert len(o["contexts"]) == len(o["quality"])
    return out


def _expected(run, prompt=(), max_tokens=-1):
    return R.contexts(list(prompt), N_TEXT_CTX, R.windows_of(run["tokens"], run["quality"]), max_tokens)


def _bits(x):
    return struct.pack("<f", float(x))


def test_contexts_follow_the_rule_and_reach_the_decoder(E, recs, oracle_tokens, tmp_models):
    eng = _engine(E, tmp_models("micro"), oracle_tokens)
    off = _alone(E, eng, recs[1])
    assert off["contexts"] == [[] for _ in off["quality"]]
    eng.set_carry_context()
    on = _alone(E, eng, recs[1])
    n = len(on["quality"])
    assert n >= 3 and any(q["seek_delta"] != 3000 for q in on["quality"])
    # window 0 has no context and is the carry-off window 0
    assert on["contexts"][0] == []
    n0 = on["quality"][0]["n_tokens"]
    assert on["quality"][0] == off["quality"][0] and on["tokens"][:n0] == off["tokens"][:off["quality"][0]["n_tokens"]]
    assert on["contexts"] == _expected(on)
    assert all(len(c) > 0 for c in on["contexts"][1:]) and any(t > oracle_tokens[0] for c in on["contexts"] for t in c)
    # the context reached the decoder: some later window scores differently
    k = min(n, len(off["quality"]))
    print(f"\navg_logprob off {[q['avg_logprob'] for q in off['quality']]}\n            on  {[q['avg_logprob'] for q in on['quality']]}")
    assert any(_bits(on["quality"][i]["avg_logprob"]) != _bits(off["quality"][i]["avg_logprob"]) for i in range(1, k))
    # off again: the parent's result again
    eng.set_carry_context(0)
    assert _alone(E, eng, recs[1]) == off
    eng.close()


def _replay(E, path, oracle_tokens, pcm, run, trace, contexts, first=1):
    """every window >= first of `run` decoded by hand on a state of a second context, behind contexts[k]: the tokens of the
    window's T = 0 record in the trace, and the kept prefix's log-probabilities averaging to the reported avg_logprob"""
    ctx = E.Context.from_file(path, 0, E.OHW_DTYPE_F16)
    st = E.State(ctx, LB.MAX_BATCH)
    st.set_batch_invariant(True)
    st.set_logit_bias(_bias(oracle_tokens))
    st.recording_set(pcm)
    p = ctx.default_params()
    p.lang_id = E.lang_code_to_id("en")
    seek, checked = 0, 0
    for k, q in enumerate(run["quality"]):
        if k >= first:
            st.mel_seek([seek], want=False)
            st.encode(1)
            st.set_window_prompt([contexts[k]] if contexts[k] else None)
            g = st.greedy_ex(1, p)[0]
            t0 = [t for (w, temp, t) in trace if w == k and temp == 0.0]
            assert len(t0) == 1
            assert g["tokens"] + ([ctx.tok.eot] if g["ended_by_eot"] else []) == t0[0], k
            if q["temperature"] == 0.0 and q["result_len"] > 0:
                s = 0.0
                for x in g["logprobs"][:q["result_len"]]:
                    s += float(x)
                assert _bits(np.float32(s / q["result_len"])) == _bits(q["avg_logprob"]), k
                checked += 1
            elif q["temperature"] == 0.0:
                assert q["avg_logprob"] == -np.inf, k          # a pass without a timestamp has no scored prefix
        seek += q["seek_delta"] if q["seek_delta"] > 0 else 3000
    st.close()
    ctx.close()
    return checked


def test_every_window_replayed_by_hand(E, recs, oracle_tokens, tmp_models):
    path = tmp_models("micro")
    eng = _engine(E, path, oracle_tokens, temperature_inc=0.0)
    eng.set_carry_context()
    on = _alone(E, eng, recs[1])
    trace = eng.last_trace()
    assert len(on["quality"]) >= 3 and all(len(c) > 0 for c in on["contexts"][1:])
    assert _replay(E, path, oracle_tokens, recs[1], on, trace, on["contexts"]) >= 1
    eng.close()


def test_long_batch_equals_every_recording_alone(E, recs, oracle_tokens, tmp_models):
    eng = _engine(E, tmp_models("micro"), oracle_tokens)
    eng.set_carry_context()
    alone = [_alone(E, eng, p) for p in recs]
    LB._check_lone_runs_make_it_a_test(alone, LB.MAX_BATCH)
    for a in alone:
        assert a["contexts"] == _expected(a)
        assert not a["contexts"] or a["contexts"][0] == []       # also in a slot another recording held before
    assert any(len(c) > 0 for a in alone for c in a["contexts"])
    together = _together(E, eng, recs)
    for i in range(len(recs)):
        assert together[i]["contexts"] == alone[i]["contexts"], i
        assert together[i]["tokens"] == alone[i]["tokens"], i
        assert together[i] == alone[i], i
    perm = [3, 0, 4, 2, 1]
    assert _together(E, eng, [recs[i] for i in perm]) == [together[i] for i in perm]
    # carry off: the contexts are gone and the tokens are another run's
    eng.set_carry_context(0)
    cold = _together(E, eng, recs)
    assert all(c == [] for t in cold for c in t["contexts"]) and [t["tokens"] for t in cold] != [t["tokens"] for t in together]
    eng.close()


def test_initial_prompt_seeds_the_history(E, recs, oracle_tokens, tmp_models):
    path = tmp_models("micro")
    prompt = [5, 6, 7, 8, 9, 10, 11] * 4
    eng = _engine(E, path, oracle_tokens)
    eng.set_initial_prompt(prompt)
    # carry off: the parent's behaviour, the prompt in front of every window - read back, and replayed by hand
    off = _alone(E, eng, recs[1])
    assert len(off["quality"]) >= 3 and off["contexts"] == [prompt] * len(off["quality"])
    assert _replay(E, path, oracle_tokens, recs[1], off, eng.last_trace(), off["contexts"], first=0) >= 1
    eng.set_carry_context()
    on = _alone(E, eng, recs[1])
    assert on["contexts"][0] == prompt
    kept0 = on["tokens"][:on["quality"][0]["n_tokens"]]
    assert len(kept0) > 0 and on["contexts"][1] == (prompt + kept0)[-CAP:]
    assert on["contexts"] == _expected(on, prompt)
    assert on["contexts"][-1] != prompt
    # a prompt of more than the cap: the engine clips it, and the clipped prompt is the seed
    long_prompt = [int(t) for t in np.random.default_rng(3).integers(1, 5000, size=CAP + 20)]
    eng.set_initial_prompt(long_prompt)
    on2 = _alone(E, eng, recs[0])
    assert on2["contexts"][0] == long_prompt[-CAP:] and on2["contexts"] == _expected(on2, long_prompt[-CAP:])
    eng.close()


def test_max_tokens_limits_every_context(E, recs, oracle_tokens, tmp_models):
    eng = _engine(E, tmp_models("micro"), oracle_tokens)
    eng.set_carry_context(3)
    on = _alone(E, eng, recs[1])
    assert len(on["quality"]) >= 3
    wins = R.windows_of(on["tokens"], on["quality"])
    hist = []
    for k, c in enumerate(on["contexts"]):
        assert len(c) <= 3 and c == hist[-3:], k
        assert k == 0 or len(c) == 3
        hist = ([] if wins[k][1] >= 0.5 else hist) + wins[k][0]
    assert on["contexts"] == _expected(on, max_tokens=3)
    eng.close()


@pytest.mark.parametrize("policy", ["last_rung", "inc_0.4"])
def test_ladder_clears_the_history(E, recs, oracle_tokens, tmp_models, policy):
    runs = []
    for device_ladder in (False, True):
        eng = _engine(E, tmp_models("micro"), oracle_tokens, temperature_inc=None, device_ladder=device_ladder)
        if policy == "last_rung":
            eng.set_decode_policy(entropy_thold=100.0)           # every pass fails the entropy test: kept at the last rung
        else:
            eng.set_decode_policy(temperature_inc=0.4)           # rungs 0.4 (behind the context) and 0.8 (without)
        eng.set_carry_context()
        runs.append(_together(E, eng, [recs[1], recs[0]]))
        one = _alone(E, eng, recs[1])
        assert one == runs[-1][0]
        eng.close()
    host, dev = runs
    temps = [[round(q["temperature"], 3) for q in r["quality"]] for r in host]
    print(f"\n{policy}: kept temperatures {temps}")
    for r in host:
        assert len(r["quality"]) >= 2
        wins = R.windows_of(r["tokens"], r["quality"])
        assert r["contexts"] == _expected(r)
        if policy == "last_rung":
            assert all(abs(q["temperature"] - 1.0) < 1e-5 for q in r["quality"])
            assert r["contexts"] == [[]] + [w[0][-CAP:] for w in wins[:-1]]
        else:
            assert all(t in (0.0, 0.4, 0.8) for t in temps[host.index(r)])
    if policy == "inc_0.4":
        flat = [t for ts in temps for t in ts]
        assert any(t > 0 for t in flat)                          # the ladder ran
    # host against device ladder: the same passes are kept, with the same tokens, contexts, seeks and segments.  The two ladders
    # score a sampled token in different places (ohw_sample_host on the host, the sampler kernel on the device): two fp32
    # log-sum-exps over the vocabulary in different orders, so the float fields of a quality record may differ in their last bits
    for i, (hr, dr) in enumerate(zip(host, dev)):
        fl = ("avg_logprob", "entropy", "no_speech_prob", "temperature")
        worst = max([abs(hq[k] - dq[k]) for hq, dq in zip(hr["quality"], dr["quality"]) for k in fl if np.isfinite(hq[k]) or np.isfinite(dq[k])] or [0.0])
        print(f"{policy}: recording {i}: host / device tokens equal {hr['tokens'] == dr['tokens']}, contexts equal {hr['contexts'] == dr['contexts']}, "
              f"largest float difference in the quality records {worst:.3e}")
    for hr, dr in zip(host, dev):
        assert hr["tokens"] == dr["tokens"] and hr["contexts"] == dr["contexts"] and hr["text"] == dr["text"]
        assert hr["segments"] == dr["segments"]
        for hq, dq in zip(hr["quality"], dr["quality"]):
            for k in hq:
                if isinstance(hq[k], float):
                    assert hq[k] == dq[k] or abs(hq[k] - dq[k]) <= FLOAT_TOL, k
                else:
                    assert hq[k] == dq[k], k


def test_beam_search_long_batch_equals_alone(E, recs, oracle_tokens, tmp_models):
    eng = _engine(E, tmp_models("micro"), oracle_tokens, max_batch=4)
    eng.set_beam_size(2)
    eng.set_carry_context()
    pcms = [recs[0], recs[2], recs[1]]
    alone = [_alone(E, eng, p) for p in pcms]
    assert sum(1 for a in alone if a["quality"]) > 2 and any(len(c) > 0 for a in alone for c in a["contexts"])
    for a in alone:
        assert a["contexts"] == _expected(a)
    together = _together(E, eng, pcms)
    for i in range(len(pcms)):
        assert together[i]["tokens"] == alone[i]["tokens"], i
        assert together[i] == alone[i], i
    eng.close()


def test_no_effect_where_every_cut_is_its_own_call(E, recs, oracle_tokens, tmp_models):
    eng = _engine(E, tmp_models("micro"), oracle_tokens)
    eng.set_schedule(E.OHW_SCHEDULE_SEQUENTIAL)
    shorts = [E.AudioBuffer(recs[3].copy(), 16000), E.AudioBuffer(recs[4].copy(), 16000), E.AudioBuffer(recs[3][:100000].copy(), 16000)]

    def fixed():
        r = eng.transcribe(E.AudioBuffer(recs[1].copy(), 16000))
        out = (r.text, eng.last_tokens(), eng.last_quality_ex(), eng.last_segments(), eng.last_contexts())
        eng.transcribe_batch(shorts)
        return out, [eng.batch_result(i) for i in range(len(shorts))]
    off = fixed()
    assert len(off[0][2]) >= 3 and all(c == [] for c in off[0][4])
    eng.set_carry_context()
    assert fixed() == off
    eng.set_carry_context(5)
    assert fixed() == off
    eng.close()


def test_refusals(E, recs, oracle_tokens, tmp_models):
    eng = _engine(E, tmp_models("micro"), oracle_tokens)
    with pytest.raises(E.WhisperError) as ex:
        eng.set_carry_context(-2)
    assert ex.value.code == E.OHW_E_INVALID_ARG
    p, n = C.POINTER(C.c_int32)(), C.c_int(0)
    assert E.lib().ohw_engine_last_context(eng.h, 0, C.byref(p), C.byref(n)) == E.OHW_E_INVALID_ARG      # nothing transcribed yet
    eng.set_window_mode(E.OHW_WINDOW_SEEK)
    eng.set_carry_context()
    eng.transcribe(E.AudioBuffer(recs[3].copy(), 16000))
    nw = len(eng.last_quality_ex())
    assert nw >= 1 and E.lib().ohw_engine_last_context(eng.h, nw - 1, C.byref(p), C.byref(n)) == 0
    for bad in (-1, nw):
        assert E.lib().ohw_engine_last_context(eng.h, bad, C.byref(p), C.byref(n)) == E.OHW_E_INVALID_ARG
    eng.transcribe_long_batch([E.AudioBuffer(recs[3].copy(), 16000)])
    assert E.lib().ohw_engine_long_batch_context(eng.h, 0, 0, C.byref(p), C.byref(n)) == 0
    for rec, win in ((1, 0), (-1, 0), (0, len(eng.long_batch_quality(0))), (0, -1)):
        assert E.lib().ohw_engine_long_batch_context(eng.h, rec, win, C.byref(p), C.byref(n)) == E.OHW_E_INVALID_ARG
    eng.close()
