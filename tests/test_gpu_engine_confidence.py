"""Confidence through the engine (ohw_engine_set_confidence): off changes and allocates nothing; on, every output of a
transcribe stays what it was and the token / word / segment records are ohw_state_score's on the kept text tokens, bit for bit,
with and without word timestamps; a hard command list shows what the feature is for; then the remaining paths - the short batch,
the long batch, the pool, the streaming session and score().  Micro model (f16)."""
import math

import numpy as np
import pytest

import command_words as W
from openhush_amd import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EOT = 50257
HEADS = [(0, 1), (1, 3)]
# one long phrase: every node of the list's trie but the last has ONE child and ends no phrase
LIST = [[47018, 17019, 20198, 8911, 11308, 47018, 17019, 20198, 8911, 11308, 47018, 17019]]


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from openhush_amd import engine
    assert hasattr(engine.lib(), "ohw_engine_set_confidence")
    return engine


def _recording():
    return np.concatenate([synth.synth_audio(21), synth.synth_audio(22), synth.synth_audio(23)])[:70 * 16000].copy()


def _engine(E, path, max_batch=3, force_len=12):
    eng = E.WhisperEngine.new(path, "en", False, True, 0, E.OHW_DTYPE_F16, max_batch)
    eng.set_decode_policy(temperature_inc=0.0, no_speech_thold=2.0)          # every window keeps its T = 0 pass
    if force_len:
        E.lib().ohw_engine_set_force_len(eng.h, force_len)
    eng.set_schedule(E.OHW_SCHEDULE_SEQUENTIAL)
    return eng


def _outputs(eng, r):
    return dict(text=r.text, tokens=eng.last_tokens(), times=eng.last_token_times(), words=eng.last_words(), segments=eng.last_segments(),
                quality=eng.last_quality_ex(), trace=eng.last_trace())


def _windows(eng):
    toks, out, i = eng.last_tokens(), [], 0
    for q in eng.last_quality_ex():
        out.append(toks[i:i + q["n_tokens"]])
        i += q["n_tokens"]
    return out


def _f32(x):
    return np.float32(x).view(np.uint32)


def _check_against_the_state(E, eng, wins, probs, word_probs, raw):
    """the records against State.score on the kept text tokens on the engine's own state (its cross K/V still holds the windows)
    and against the two host rules"""
    st = eng.state_view()
    p = st.ctx.default_params()
    text = [[t for t in w if t < EOT] for w in wins]
    scores = st.score(text, p=p)
    k, wi = 0, 0
    for w, (toks, sc) in enumerate(zip(text, scores)):
        lpt = []
        for t, s in zip(toks, sc[:-1]):
            got = probs[k]
            lt, la, tt = E.token_prob_host(s)
            assert (got["id"], got["window"], got["top_id"]) == (t, w, int(s["top_id"])), (k, got)
            assert _f32(got["logprob_text"]) == _f32(lt) and _f32(got["logprob_all"]) == _f32(la) and _f32(got["top_logprob_text"]) == _f32(tt), (k, got)
            lpt.append(lt)
            k += 1
        tb = [st.ctx.token_text(t) for t in toks]
        starts = E.word_starts(tb)
        want = E.word_probs_host(lpt, [int(x) for x in starts])
        for j in range(len(want)):
            assert _f32(word_probs[wi + j]["probability"]) == _f32(want[j]), (w, j)
        wi += len(want)
    assert k == len(probs) and wi == len(word_probs)
    return scores


def test_off_is_the_parent_and_on_changes_no_other_output(E, tmp_models):
    path = tmp_models("micro")
    audio = E.AudioBuffer(_recording(), 16000)
    eng = _engine(E, path)
    st = eng.state_view()
    off = _outputs(eng, eng.transcribe(audio))
    assert eng.last_token_probs() == [] and eng.last_word_probs() == [] and eng.last_segment_info() == []
    assert st.counter("token_score") == 0 and st.counter("score_buffers") == 0
    gemms = st.counter("dec_gemm.total")
    eng.transcribe(audio)
    per_call = st.counter("dec_gemm.total") - gemms                          # graphs are captured: a repeat launches the prompt passes only
    # on, without word timestamps
    eng.set_confidence(True)
    on = _outputs(eng, eng.transcribe(audio))
    assert on == off
    assert st.counter("score_buffers") == 1 and st.counter("token_score") > 0 and st.counter("dec_gemm.total") - gemms - per_call > per_call
    probs, wprobs, info = eng.last_token_probs(), eng.last_word_probs(), eng.last_segment_info()
    wins = _windows(eng)
    assert len(wins) == 3 and [p["id"] for p in probs] == [t for t in on["tokens"] if t < EOT]
    assert len(info) == len(on["segments"]) > 0
    _check_against_the_state(E, eng, wins, probs, wprobs, eng._last_text_bytes())
    # logprob_decode is the kept pass's own token_logprobs: greedy_ex again on the same state, the engine's parameters
    p = st.ctx.default_params()
    p.force_len = 12; p.n_max = 12
    rows = st.greedy_ex(3, p)
    assert [list(r["tokens"])[:len(w)] for r, w in zip(rows, wins)] == wins
    dec = [lp for r, w in zip(rows, wins) for t, lp in zip(w, r["logprobs"]) if t < EOT]
    assert [_f32(a["logprob_decode"]) for a in probs] == [_f32(b) for b in dec]
    for s, i in zip(on["segments"], info):
        assert math.isfinite(i["avg_logprob"]) and i["avg_logprob"] < 0 and 0.0 <= i["no_speech_prob"] <= 1.0 and i["temperature"] == 0.0
    if len(info) == 3:                                                          # one segment per window: its mean is the window's
        for w in range(3):
            mean = np.mean([np.float64(np.float32(a["logprob_text"])) for a in probs if a["window"] == w])
            assert abs(info[w]["avg_logprob"] - mean) < 1e-6, w
    # on, with word timestamps: one replay serves both, the spans of the word probabilities are the words'
    eng.set_word_timestamps(HEADS)
    eng.set_confidence(False)
    assert st.counter("score_buffers") == 0                                     # off gives the buffers back
    timed = _outputs(eng, eng.transcribe(audio))
    assert timed["tokens"] == off["tokens"] and timed["text"] == off["text"] and timed["segments"] == off["segments"] and len(timed["words"]) > 0
    before = st.counter("dec_gemm.total"), st.counter("token_score")
    eng.transcribe(audio)
    align_only = st.counter("dec_gemm.total") - before[0]
    assert st.counter("token_score") == before[1]
    eng.set_confidence(True)
    before = st.counter("dec_gemm.total"), st.counter("token_score")
    both = _outputs(eng, eng.transcribe(audio))
    assert st.counter("dec_gemm.total") - before[0] == align_only and st.counter("token_score") > before[1]
    assert both == timed
    assert eng.last_token_probs() == probs and eng.last_segment_info() == info
    wp = eng.last_word_probs()
    assert [(w["text_off"], w["text_len"]) for w in wp] == [(w["text_off"], w["text_len"]) for w in both["words"]]
    assert [w["probability"] for w in wp] == [w["probability"] for w in wprobs]
    eng.close()


def test_a_hard_command_list_is_what_the_feature_is_for(E, tmp_models, tmp_path):
    """A forced token - the only column the filtered row leaves - has a decode log-probability of about 0 whatever the audio;
    logprob_text is the unconstrained model's score of the same token.  Forced, from the rule and the sampler's filter and not
    from the result: the token is the sole child of its node, the node ends no phrase (end-of-text is lowered there), and the two
    tokens in front of it are timestamps, where the sampler's pairing rule bans every timestamp.  A sole child anywhere else is
    NOT forced: the rule never touches timestamps, and an opening or closing timestamp competes with it - measured on an MI355X:
    logprob_decode of 17019 behind 47018 was -0.263, -0.268 and -0.467 in the three windows (logprob_text -4.90, -4.47, -5.53)."""
    path = W.worded_model(tmp_models("micro"), str(tmp_path / "ggml-micro-words.bin"))
    eng = _engine(E, path, max_batch=3, force_len=0)
    eng.set_commands(LIST, math.inf)
    eng.set_confidence(True)
    eng.transcribe(E.AudioBuffer(_recording(), 16000))
    wins, probs = _windows(eng), eng.last_token_probs()
    assert len(wins) == 3 and all(LIST[0][:len([t for t in w if t < EOT])] == [t for t in w if t < EOT] for w in wins), wins
    # the rules live on the engine's own state: scoring there must still be the unconstrained model's
    st = eng.state_view()
    assert st.command_count() == len(LIST)
    _check_against_the_state(E, eng, wins, probs, eng.last_word_probs(), eng._last_text_bytes())
    ts0 = st.ctx.tok.timestamp_begin
    forced, others, k = [], [], 0
    for w in wins:
        for i, t in enumerate(w):
            if t >= EOT:
                continue
            depth = len([x for x in w[:i] if x < EOT])                          # the node: depth < len(phrase), so one child, no phrase ends
            (forced if i >= 2 and w[i - 1] >= ts0 and w[i - 2] >= ts0 and depth < len(LIST[0]) else others).append(probs[k])
            k += 1
    print("windows:", wins)
    print("forced tokens:", [(f["id"], round(f["logprob_decode"], 6), round(f["logprob_text"], 4)) for f in forced])
    print("the others:", [(f["id"], round(f["logprob_decode"], 4), round(f["logprob_text"], 4)) for f in others])
    assert forced, wins
    for f in forced:
        assert f["logprob_decode"] > -1e-3, f
    assert any(f["logprob_text"] < -0.05 for f in probs)                          # the model itself was not that sure
    eng.close()


def test_short_batch_long_batch_and_score(E, tmp_models):
    path = tmp_models("micro")
    audios = [E.AudioBuffer(synth.synth_audio(50 + i, 16000 * (8 + 7 * i)), 16000) for i in range(3)]
    eng = _engine(E, path)
    eng.set_confidence(True)
    res = eng.transcribe_batch(audios)
    kept = []
    for i, r in enumerate(res):
        toks = eng.batch_result(i)[1]
        kept.append([t for t in toks if t < EOT])
        assert [p["id"] for p in r.token_probs] == kept[i] and len(r.word_probs) > 0 and len(r.segment_info) == len(r.segments)
        assert all(p["window"] == 0 for p in r.token_probs)
    # recording i of the batch equals recording i alone
    for i in range(3):
        alone = eng.transcribe_batch([audios[i]])[0]
        assert alone.token_probs == res[i].token_probs and alone.word_probs == res[i].word_probs and alone.segment_info == res[i].segment_info, i
    # score() of a recording's own kept tokens is that transcribe's list (logprob_decode apart: nothing is decoded)
    eng.set_confidence(False)
    sc = eng.score(audios, kept)
    for i in range(3):
        strip = lambda ps: [{k: v for k, v in p.items() if k != "logprob_decode"} for p in ps]
        assert strip(sc[i]["tokens"]) == strip(res[i].token_probs), i
        assert all(math.isnan(p["logprob_decode"]) for p in sc[i]["tokens"])
        assert sc[i]["eot"]["id"] == EOT and math.isfinite(sc[i]["eot"]["logprob_all"])
        want = float(np.float32(sum(np.float64(np.float32(p["logprob_all"])) for p in sc[i]["tokens"] + [sc[i]["eot"]])))
        assert sc[i]["sum_logprob"] == want
    other = eng.score(audios[:1], [[(kept[0][0] + 1) % EOT] + kept[0][1:]])
    assert other[0]["sum_logprob"] != sc[0]["sum_logprob"]
    with pytest.raises(E.WhisperError):
        eng.score(audios[:1], [[EOT]])
    with pytest.raises(E.WhisperError):
        eng.score(audios[:1], [[1] * 225])
    # the long batch equals the seek loop, recording by recording
    eng.set_confidence(True)
    long_audios = [E.AudioBuffer(_recording()[:16000 * 40], 16000), audios[2]]
    lb = eng.transcribe_long_batch(long_audios)
    eng.set_window_mode(E.OHW_WINDOW_SEEK)
    st = eng.state_view()
    for i, a in enumerate(long_audios):
        st.set_batch_invariant(True)
        r = eng.transcribe(a)
        st.set_batch_invariant(False)
        assert r.text == lb[i].text
        assert eng.last_token_probs() == lb[i].token_probs and eng.last_word_probs() == lb[i].word_probs and eng.last_segment_info() == lb[i].segment_info, i
    eng.close()


def test_pool_gathers_in_recording_order(E, tmp_models):
    path = tmp_models("micro")
    audio = E.AudioBuffer(_recording(), 16000)
    eng = _engine(E, path, max_batch=1)
    eng.set_confidence(True)
    ref = eng.transcribe(audio)
    one = dict(tokens=eng.last_tokens(), probs=eng.last_token_probs(), words=eng.last_word_probs(), info=eng.last_segment_info())
    eng.close()
    pool = E.EnginePool(path, "en", False, [0, 0], E.OHW_DTYPE_F16, 1)
    pool.set_decode_policy(temperature_inc=0.0, no_speech_thold=2.0)
    pool.set_force_len(12)
    pool.set_schedule(E.OHW_SCHEDULE_SEQUENTIAL)
    r = pool.transcribe(audio)
    assert pool.last_token_probs() == [] and pool.last_word_probs() == [] and pool.last_segment_info() == []
    pool.set_confidence(True)
    r = pool.transcribe(audio)
    assert r.text == ref.text and pool.last_tokens() == one["tokens"]
    got = pool.last_token_probs()
    assert [(p["id"], p["window"]) for p in got] == [(p["id"], p["window"]) for p in one["probs"]] and sorted({p["window"] for p in got}) == [0, 1, 2]
    # one window per batch on either side and the same kernels: the same words
    assert got == one["probs"] and pool.last_word_probs() == one["words"] and pool.last_segment_info() == one["info"]
    pool.set_confidence(False)
    pool.transcribe(audio)
    assert pool.last_token_probs() == []
    pool.close()


def test_streaming_session_carries_the_lists(E):
    from openhush_amd import streaming as S
    ctx = E.Context.synthetic(synth.PRESETS["micro"].as_list(), 1234, 0, E.OHW_DTYPE_F16)
    p = ctx.default_params(); p.n_max = 16
    rec = synth.synth_audio(31)[:16000 * 5]
    plain = S.StreamingSession(ctx, beam_size=0, params=p).tick(rec, len(rec), is_final=True)
    assert plain[0].token_probs == [] and plain[0].word_probs == []
    ses = S.StreamingSession(ctx, beam_size=0, params=p, confidence=True)
    out = ses.tick(rec, len(rec), is_final=True)
    assert len(out) == 1 and out[0].text == plain[0].text
    tp, wp = out[0].token_probs, out[0].word_probs
    assert len(tp) > 0 and len(wp) > 0 and all(t["id"] < EOT and t["logprob_text"] <= 0.0 and t["logprob_all"] <= t["logprob_text"] + 1e-6 for t in tp)
    assert all(0.0 <= w["probability"] <= 1.0 and w["text_len"] > 0 for w in wp)
    assert "".join(w["text"] for w in wp).strip() == out[0].text
    sc = ses.state.score([[t["id"] for t in tp]], p=p)[0]
    assert [_f32(t["logprob_text"]) for t in tp] == [_f32(E.token_prob_host(s)[0]) for s in sc[:-1]]
