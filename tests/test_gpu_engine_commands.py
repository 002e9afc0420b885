"""Command lists through the engine (ohw_engine_set_commands): transcribe on the engine's own state and on lanes,
transcribe_batch, a forced host-sampled ladder against the device-sampled one, and a pool with one device listed twice.
Micro model (f16).  Every list is hard (p = +inf), so a kept window's text tokens are one listed phrase by construction, and
last_commands() must name it as ohw_command_match_host does.
"""
import math

import numpy as np
import pytest

import command_words as W
from openhush_amd import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EOT = 50257
LIST = [[47018, 17019], [47018, 17019, 20198], [8911], [11308, 8911, 47018], [17019, 17019, 17019], [20198, 11308], [47018, 17019]]


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from openhush_amd import engine
    engine.lib()
    return engine


def _windows(eng):
    """the kept tokens of the last transcribe, per window"""
    toks, out, i = eng.last_tokens(), [], 0
    for q in eng.last_quality_ex():
        out.append(toks[i:i + q["n_tokens"]])
        i += q["n_tokens"]
    assert i == len(toks)
    return out


def _text(tokens):
    return [t for t in tokens if t < EOT]


def _check_hits(E, hits, wins, phrases=LIST, index=None):
    """one hit per window, in window order; the phrase is what ohw_command_match_host finds in the window's kept tokens"""
    table = E.command_table_build_host(phrases, EOT)
    assert [h["window"] for h in hits] == list(range(len(wins)))
    for h, w in zip(hits, wins):
        k = E.command_match_host(table, w)
        assert h["index"] == (-1 if k < 0 else index[k] if index else k), (h, w)
        assert math.isfinite(h["list_logprob"]) and h["list_logprob"] < 0, h


def test_transcribe_on_lanes_and_on_the_engines_own_state(E, tmp_models):
    path = tmp_models("micro")
    pcm = np.concatenate([synth.synth_audio(40 + w) for w in range(3)])[:16000 * 70]

    def run(schedule):
        eng = E.WhisperEngine.new(path, "en", False, True, 0, E.OHW_DTYPE_F16, 1)
        eng.set_decode_policy(temperature_inc=0.0, no_speech_thold=2.0)          # every window keeps its T = 0 pass
        eng.set_schedule(schedule, lanes=2, merge=1)
        eng.transcribe(E.AudioBuffer(pcm.copy(), 16000))
        plain, none = _windows(eng), eng.last_commands()
        eng.set_commands(LIST, math.inf)
        eng.transcribe(E.AudioBuffer(pcm.copy(), 16000))
        wins, hits = _windows(eng), eng.last_commands()
        eng.set_commands(None)
        eng.transcribe(E.AudioBuffer(pcm.copy(), 16000))
        cleared, none2 = _windows(eng), eng.last_commands()
        eng.close()
        assert none == [] and none2 == [] and cleared == plain
        return plain, wins, hits
    plain, own, own_hits = run(E.OHW_SCHEDULE_SEQUENTIAL)
    _, lanes, lane_hits = run(E.OHW_SCHEDULE_LANES)
    assert len(own) == 3 and own != plain and own == lanes
    assert all(_text(w) in LIST for w in own), own
    _check_hits(E, own_hits, own)
    _check_hits(E, lane_hits, lanes)
    assert all(h["index"] >= 0 for h in own_hits) and [h["index"] for h in own_hits] == [h["index"] for h in lane_hits]
    assert all(h["index"] != 6 for h in own_hits)                                # of the duplicates 0 and 6, the lower index
    # bad values reach no state
    eng = E.WhisperEngine.new(path, "en", False, True, 0, E.OHW_DTYPE_F16, 1)
    try:
        for bad in (dict(phrases=LIST, penalty=0.0), dict(phrases=LIST, penalty=float("nan")), dict(phrases=[[EOT]]), dict(phrases=[[1] * 17])):
            with pytest.raises(E.WhisperError) as ex:
                eng.set_commands(**bad)
            assert ex.value.code == E.OHW_E_INVALID_ARG
        eng.transcribe(E.AudioBuffer(pcm[:16000 * 20].copy(), 16000))
        assert eng.last_commands() == []
    finally:
        eng.close()


@pytest.fixture(scope="module")
def worded(E, tmp_models, tmp_path_factory):
    """the micro model under a vocabulary with a few words in it -> (its path, a context on it)"""
    path = W.worded_model(tmp_models("micro"), str(tmp_path_factory.mktemp("worded") / "ggml-micro-words.bin"))
    return path, E.Context.from_file(path, 0, E.OHW_DTYPE_F16)


def test_transcribe_batch_text_form_and_both_forms_share_an_index(E, worded):
    path, ctx = worded
    phrases = list(W.PHRASES)
    forms, index = E.command_tokens(ctx, phrases)
    assert forms == W.FORMS and index == W.INDEX                                 # a text is listed as given and with a leading space
    eng = E.WhisperEngine.new(path, "en", False, True, 0, E.OHW_DTYPE_F16, 3)
    eng.set_decode_policy(temperature_inc=0.0, no_speech_thold=2.0)
    eng.set_commands(phrases, math.inf)
    audios = [E.AudioBuffer(synth.synth_audio(50 + i, 16000 * (8 + 7 * i)), 16000) for i in range(3)]
    res = eng.transcribe_batch(audios)
    for i, r in enumerate(res):
        text, toks, q, _ = eng.batch_result(i)
        hits = eng.last_commands(i)
        _check_hits(E, hits, [toks], forms, index)
        assert len(hits) == 1 and hits[0]["index"] >= 0 and _text(toks) in forms
        assert r.text.strip() == phrases[hits[0]["index"]]
    with pytest.raises(E.WhisperError):
        eng.last_commands(3)
    eng.close()


def test_host_sampled_ladder_obeys_the_list_as_the_device_sampled_one_does(E, tmp_models):
    """logprob_thold 0 rejects every pass, so each window climbs the whole ladder; on the host it applies ohw_command_rule_host,
    on the device the kernel: the same passes, the same kept tokens, list_logprob of the kept pass alike"""
    path = tmp_models("micro")
    pcm = np.concatenate([synth.synth_audio(40 + w) for w in range(2)])
    prefixes = {tuple(p[:d]) for p in LIST for d in range(len(p) + 1)}

    def run(on_device):
        eng = E.WhisperEngine.new(path, "en", False, True, 0, E.OHW_DTYPE_F16, 2)
        eng.set_decode_policy(logprob_thold=0.0, no_speech_thold=2.0)
        eng.set_fallback_on_device(on_device)
        eng.set_commands(LIST, math.inf)
        eng.transcribe(E.AudioBuffer(pcm.copy(), 16000))
        out = eng.last_trace(), _windows(eng), eng.last_commands(), [q["temperature"] for q in eng.last_quality_ex()]
        eng.close()
        return out
    trace, kept, hits, temps = run(False)
    assert sorted({round(T, 1) for _, T, _ in trace})[-1] >= 0.8 and all(T > 0.0 for T in temps)      # the kept pass came from the ladder
    for w, T, toks in trace:
        assert tuple(_text(toks)) in prefixes, (w, T, toks)                      # a pass cut short is still on the list
    assert len(kept) == 2 and all(_text(k) in LIST for k in kept), kept
    _check_hits(E, hits, kept)
    trace_d, kept_d, hits_d, temps_d = run(True)
    assert kept_d == kept and temps_d == temps and [h["index"] for h in hits_d] == [h["index"] for h in hits]
    # the host sums in double, the kernel in float32 (command_ref.lp_tol: 2.2e-5 at this vocabulary and |logit| <= 20); the two
    # ladders' logits differ by the decoder's own batch shapes, which moves a log-probability in the fourth decimal at most
    assert np.allclose([h["list_logprob"] for h in hits_d], [h["list_logprob"] for h in hits], atol=2e-3), (hits_d, hits)


def test_pool_with_one_device_listed_twice(E, worded):
    path, ctx = worded
    phrases, forms = list(W.PHRASES), W.FORMS
    pcm = np.concatenate([synth.synth_audio(70 + w) for w in range(3)] + [synth.synth_audio(75, 90000)])
    eng = E.WhisperEngine.new(path, "en", False, True, 0, E.OHW_DTYPE_F16, 1)
    eng.set_decode_policy(temperature_inc=0.0, no_speech_thold=2.0)
    eng.set_schedule(E.OHW_SCHEDULE_SEQUENTIAL)
    eng.set_commands(phrases, math.inf)
    ref = eng.transcribe(E.AudioBuffer(pcm, 16000))
    ref_tokens, ref_wins = eng.last_tokens(), _windows(eng)
    eng.close()
    assert len(ref_wins) == 4 and all(_text(w) in forms for w in ref_wins)
    pool = E.EnginePool(path, "en", False, [0, 0], E.OHW_DTYPE_F16, 1)
    pool.set_decode_policy(temperature_inc=0.0, no_speech_thold=2.0)
    pool.set_schedule(E.OHW_SCHEDULE_SEQUENTIAL)
    pool.set_commands(phrases, math.inf)
    res = pool.transcribe(E.AudioBuffer(pcm, 16000))
    assert res.text == ref.text and pool.last_tokens() == ref_tokens
    pool.set_commands(None)
    plain = pool.transcribe(E.AudioBuffer(pcm, 16000))
    assert plain.text != ref.text
    with pytest.raises(ValueError):
        pool.set_commands([[1, 2]])
    with pytest.raises(E.WhisperError):
        pool.set_commands(phrases, -1.0)
    pool.close()


@pytest.mark.parametrize("beam", [0, 3])
def test_streaming_session_holds_every_chunk_to_the_list(E, worded, beam):
    """StreamingSession(commands=..., command_penalty=inf): a chunk's text is a listed phrase, last_command names it with the
    caller's index, last_list_logprob is the state's value; without the option nothing is set"""
    from openhush_amd import streaming as S
    path, ctx = worded
    phrases = list(W.PHRASES)
    p = ctx.default_params(); p.n_max = 24
    rec = synth.synth_audio(31)[:16000 * 5]
    plain = S.StreamingSession(ctx, beam_size=beam, params=p)
    out0 = plain.tick(rec, len(rec), is_final=True)
    assert plain.state.command_count() == 0 and plain.last_command == -1 and math.isnan(plain.last_list_logprob)
    ses = S.StreamingSession(ctx, beam_size=beam, params=p, commands=phrases, command_penalty=math.inf)
    assert ses.state.command_count() == len(W.FORMS)
    out = ses.tick(rec, len(rec), is_final=True)
    assert len(out) == 1 and out[0].text in phrases and out[0].text != out0[0].text
    assert ses.last_command == phrases.index(out[0].text)
    assert math.isfinite(ses.last_list_logprob) and ses.last_list_logprob < 0
    with pytest.raises(ValueError):
        S.StreamingSession(ctx, beam_size=beam, params=p, commands=phrases, command_penalty=0.0)
