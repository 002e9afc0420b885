"""Stitched windows through the engine (ohw_engine_set_stitch): off after on is a fresh engine; a window of the plan is the
window transcribed alone; tokens, text, segments and seams are the Python restatement (tests/stitch_ref.py) applied to those
windows, in every schedule and both fixed-cut modes; the seek loop ignores the setting; token times and probabilities list the
retained text tokens.  Micro model (f16), max_batch 4, batch-invariant kernels, recordings of 3 to 5 windows."""
import numpy as np
import pytest

import stitch_ref as S
from openhush_amd import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EOT = 50257
HEADS = [(0, 1), (1, 3)]
OVERLAP_S = 5.0
HOP = 480000 - 5000 * 16


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from openhush_amd import engine
    assert hasattr(engine.lib(), "ohw_engine_set_stitch")
    return engine


def _recording(seconds, first=40):
    n = int(seconds * 16000)
    return np.concatenate([synth.synth_audio(first + k) for k in range(-(-n // 480000))])[:n].copy()


def _engine(E, path, mode=None, schedule=None, stitch=OVERLAP_S, times=False):
    eng = E.WhisperEngine.new(path, "en", False, True, 0, E.OHW_DTYPE_F16, 4)
    eng.set_decode_policy(temperature_inc=0.0, no_speech_thold=2.0)          # every window keeps its T = 0 pass
    # 24 tokens a window; a bias that lets timestamps compete and no repeated token: the micro model's text then follows the
    # audio (five different windows in the 118 s recording, seams of 2 to 6 matches), with timestamp tokens between the text
    eng.set_force_len(24)
    st = eng.state_view()
    bias = np.zeros(st.ctx.hp.n_vocab, np.float32)
    bias[st.ctx.tok.timestamp_begin:] = 6.0
    bias[st.ctx.tok.eot] = 27.0
    st.set_logit_bias(bias)
    eng.set_repetition(1.0, 1)
    eng.set_window_mode(E.OHW_WINDOW_FIXED if mode is None else mode)
    eng.set_schedule(*(schedule or (E.OHW_SCHEDULE_SEQUENTIAL, 0, 0)))
    if times:
        eng.set_word_timestamps(HEADS)
        eng.set_confidence(True)
    if stitch:
        eng.set_stitch(stitch)
    return eng


def _out(eng, r):
    return dict(text=r.text, tokens=eng.last_tokens(), segments=eng.last_segments(), seams=eng.last_seams(), windows=eng.last_window_tokens(),
                quality=eng.last_quality_ex(), trace=eng.last_trace())


def _run(E, path, pcm, **kw):
    eng = _engine(E, path, **kw)
    out = _out(eng, eng.transcribe(E.AudioBuffer(pcm, 16000)))
    eng.close()
    return out


def _check_against_the_restatement(E, eng_ctx, out, n):
    """tokens, text, segments and seams of a stitched transcribe against the restatement applied to its own windows"""
    wins = out["windows"]
    hop, W, spans = S.plan(n, int(OVERLAP_S * 1000))
    assert hop == HOP and len(wins) == W == len(out["quality"]) and [q["n_tokens"] for q in out["quality"]] == [len(w) for w in wins]
    sw, rg, merged = S.stitch(wins, EOT)
    assert out["tokens"] == merged
    assert [[s[k] for k in E.SEAM_WORDS[:7]] for s in out["seams"]] == sw[:, :7].tolist()
    raw = b"".join(eng_ctx.token_text(t) for t in merged if t < EOT)
    assert out["text"] == raw.strip(b" \t\r\n").decode("utf-8", "replace")
    want = []
    for w, (win, (a, b)) in enumerate(zip(wins, rg)):
        t_off, t_end = spans[w][0] / 16000.0, spans[w][1] / 16000.0
        for seg in E.segments_host(win, eng_ctx.tok, t_off, t_end):
            c = S.clip_segment(seg, a, b, S.seam_time(w - 1, hop, n) if w else 0.0, S.seam_time(w, hop, n) if w + 1 < W else 0.0)
            if c is not None:
                text = b"".join(eng_ctx.token_text(t) for t in win[c[0]:c[1]] if t < EOT)
                want.append((text.decode("utf-8", "replace").strip(), np.float32(c[2]), np.float32(c[3])))
    got = [(s["text"].strip(), np.float32(s["t0"]), np.float32(s["t1"])) for s in out["segments"]]
    assert got == want
    return sw, rg


@pytest.fixture(scope="module")
def long_case(E, tmp_models):
    """118 s: windows at 0, 25, 50, 75 and 100 s, the last of 18 s; two batches of max_batch 4.  Computed once, never changed"""
    path = tmp_models("micro")
    pcm = _recording(118)
    eng = _engine(E, path)
    out = _out(eng, eng.transcribe(E.AudioBuffer(pcm, 16000)))
    ctx = eng.state_view().ctx
    return path, pcm, out, ctx, eng


def test_off_after_on_is_a_fresh_engine(E, tmp_models):
    path = tmp_models("micro")
    pcm = _recording(70)
    fresh = _run(E, path, pcm, stitch=None)
    assert fresh["seams"] == [] and fresh["windows"] == [] and len(fresh["quality"]) == 3
    eng = _engine(E, path, stitch=None)
    assert eng.stitch() == 0.0
    eng.set_stitch(5.0)
    assert eng.stitch() == 5.0
    on = _out(eng, eng.transcribe(E.AudioBuffer(pcm, 16000)))
    assert len(on["seams"]) == 2 and len(on["windows"]) == 3
    for off_value in (0, None):
        eng.set_stitch(off_value)
        assert eng.stitch() == 0.0
        again = _out(eng, eng.transcribe(E.AudioBuffer(pcm, 16000)))
        assert again == fresh
        eng.set_stitch(5.0)
    for bad in (0.5, 15.02, 5.01, -5.0):
        with pytest.raises(E.WhisperError):
            eng.set_stitch(bad)
    assert eng.stitch() == 5.0
    eng.close()


def test_a_recording_of_one_window_has_no_seam_and_the_stitch_off_result(E, tmp_models):
    path = tmp_models("micro")
    for seconds in (20, 30):
        pcm = _recording(seconds, first=45)
        off, on = _run(E, path, pcm, stitch=None), _run(E, path, pcm)
        assert on["seams"] == [] and on["windows"] == [off["tokens"]] and len(on["quality"]) == 1
        for k in ("text", "tokens", "segments", "quality", "trace"):
            assert on[k] == off[k], k


def test_a_window_of_the_plan_is_the_window_alone_and_the_merge_is_the_restatement(E, long_case):
    path, pcm, out, ctx, _ = long_case
    lone = _engine(E, path, stitch=None)
    alone = []
    for k in range(5):
        lone.state_view().set_batch_invariant(True)                      # what a transcribe of several windows runs under
        lone.transcribe(E.AudioBuffer(pcm[k * HOP:k * HOP + 480000].copy(), 16000))
        alone.append(lone.last_tokens())
    lone.close()
    assert len(pcm) - 4 * HOP == 18 * 16000                             # the last window is short
    assert out["windows"] == alone
    assert len({tuple(w) for w in alone}) == 5                          # five different windows: an index slip would show
    sw, _ = _check_against_the_restatement(E, ctx, out, len(pcm))
    assert all(m >= 2 for m in sw[:, 2]) and any(0 < lc < n for _, _, _, lc, _, n, _, _ in sw.tolist())      # matched seams that cut


def test_audio_that_repeats_with_the_hop_matches_whole_windows(E, tmp_models):
    """every full window hears the same audio, so every seam between two full windows aligns them wholly: shift == matches ==
    n_text, the cuts at n_text / 2.  By the range rule [rc, lc) the first window then gives n_text / 2 text tokens, the last
    n_text - n_text / 2 and a window between two such seams none: together one copy of the window's text"""
    path = tmp_models("micro")
    period = synth.synth_audio(51)[:HOP]
    pcm = np.tile(period, 5)[:3 * HOP + 480000].copy()                   # four full windows
    out = _run(E, path, pcm)
    wins = out["windows"]
    assert len(wins) == 4 and wins[1] == wins[0] and wins[2] == wins[0] and wins[3] == wins[0]
    text = [t for t in wins[0] if t < EOT]
    n_text = len(text)
    assert n_text >= 2
    for s in out["seams"]:
        assert (s["shift"], s["matches"], s["left_cut"], s["right_cut"], s["n_left"], s["n_right"]) == (n_text, n_text, n_text // 2, n_text // 2, n_text, n_text)
    _, rg = _check_against_the_restatement(E, _ctx_of(E, path), out, len(pcm))
    per_window = [len([t for t in w[a:b] if t < EOT]) for w, (a, b) in zip(wins, rg)]
    assert per_window == [n_text // 2, 0, 0, n_text - n_text // 2]
    assert [t for t in out["tokens"] if t < EOT] == text


_CTX = {}


def _ctx_of(E, path):
    if path not in _CTX:
        eng = _engine(E, path, stitch=None)
        _CTX[path] = (eng, eng.state_view().ctx)                          # the engine owns the context: keep it
    return _CTX[path][1]


def test_the_schedules_and_both_fixed_modes_agree_each_with_the_restatement(E, long_case):
    path, pcm, seq_fixed, ctx, _ = long_case
    for mode in (E.OHW_WINDOW_FIXED, E.OHW_WINDOW_FIXED_RECORDING_MEL):
        outs = {}
        for name, schedule in (("sequential", (E.OHW_SCHEDULE_SEQUENTIAL, 0, 0)), ("pipeline", (E.OHW_SCHEDULE_PIPELINE, 0, 0)),
                               ("lanes", (E.OHW_SCHEDULE_LANES, 2, 1))):
            if mode == E.OHW_WINDOW_FIXED and name == "sequential":
                outs[name] = seq_fixed
                continue
            outs[name] = _run(E, path, pcm, mode=mode, schedule=schedule)
        for name in outs:
            assert outs[name] == outs["sequential"], (mode, name)
        assert len(outs["sequential"]["seams"]) == 4
        _check_against_the_restatement(E, ctx, outs["sequential"], len(pcm))


def test_the_seek_loop_ignores_the_setting(E, tmp_models):
    path = tmp_models("micro")
    pcm = _recording(70)
    off = _run(E, path, pcm, mode=E.OHW_WINDOW_SEEK, stitch=None)
    on = _run(E, path, pcm, mode=E.OHW_WINDOW_SEEK)
    assert on == off and on["seams"] == [] and on["windows"] == [] and len(on["tokens"]) > 0


def test_token_times_and_probabilities_list_the_retained_text_tokens(E, tmp_models):
    path = tmp_models("micro")
    pcm = _recording(95, first=60)                                       # windows at 0, 25, 50 and (15 s) 75 s
    eng = _engine(E, path, times=True)
    out = _out(eng, eng.transcribe(E.AudioBuffer(pcm, 16000)))
    times, probs, words, wprobs = eng.last_token_times(), eng.last_token_probs(), eng.last_words(), eng.last_word_probs()
    info, n_bytes = eng.last_segment_info(), len(eng._last_text_bytes())
    _, rg = _check_against_the_restatement(E, eng.state_view().ctx, out, len(pcm))
    eng.close()
    assert len(out["windows"]) == 4
    want = [(t, w) for w, (win, (a, b)) in enumerate(zip(out["windows"], rg)) for t in win[a:b] if t < EOT]
    assert len(want) >= 2
    assert [(t["id"], t["window"]) for t in times] == want
    assert [(p["id"], p["window"]) for p in probs] == want
    assert len(info) == len(out["segments"])
    for name, spans in (("words", words), ("word_probs", wprobs), ("segments", out["segments"])):
        for s in spans:
            assert 0 <= s["text_off"] and s["text_len"] >= 0 and s["text_off"] + s["text_len"] <= n_bytes, (name, s)
    for t in times:
        assert 25.0 * t["window"] <= t["t0"] <= t["t1"] <= min(25.0 * t["window"] + 30.0, 95.0) + 1e-3, t
    # the retained tokens' times and probabilities are those of the same windows with stitch off (a cut changes no value)
    eng = _engine(E, path, times=True, stitch=None)
    eng.state_view().set_batch_invariant(True)
    k = 1
    eng.transcribe(E.AudioBuffer(pcm[k * HOP:k * HOP + 480000].copy(), 16000))
    lone_times, lone_probs = eng.last_token_times(), eng.last_token_probs()
    eng.close()
    text_pos = [i for i, t in enumerate(out["windows"][k]) if t < EOT]
    a, b = rg[k]
    keep = [j for j, i in enumerate(text_pos) if a <= i < b]
    got_t = [t for t in times if t["window"] == k]
    got_p = [p for p in probs if p["window"] == k]
    assert [t["id"] for t in got_t] == [lone_times[j]["id"] for j in keep]
    for t, j in zip(got_t, keep):                                        # fp32 sums of an offset and a multiple of 0.02: 25 + x against 0 + x
        assert abs(t["t0"] - 25.0 * k - lone_times[j]["t0"]) < 1e-4 and abs(t["t1"] - 25.0 * k - lone_times[j]["t1"]) < 1e-4, (t, j)
    assert [{**p, "window": 0} for p in got_p] == [lone_probs[j] for j in keep]
