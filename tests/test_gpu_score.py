"""ohw_state_score on the GPU: the teacher-forced confidence pass over a window's text tokens (include/ohw.h, "confidence").

Against the oracle: State.decode(seq, 0, all_pos=True) on the GPU's own encoder output gives every position's raw logits,
tests/score_ref.py turns them into scores.  logit, top_logit, logit - lse_text and logit - lse_all are each held to
2 x TOL_LOGIT of tests/test_gpu_prompt.py (a log-soft-max moves by at most twice the largest logit error); top_id is judged by
value: the reference row at the device's top_id lies within 2 x TOL_LOGIT of the reference maximum over the text columns.
Everything else is bit equality: the kept logits rows, score-only against score-with-align, the alignment against
ohw_state_align, a window alone against the window in a batch, and every decode mode after a score against a fresh state."""
import numpy as np
import pytest

from openhush_amd import synth

import score_ref as R
import state_modes as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MICRO = synth.PRESETS["micro"]
TOL_LOGIT = {0: 0.25, 1: 0.03}           # tests/test_gpu_prompt.py
N_TEXT = [0, 1, 4, 60]                   # P = 4: 4 tokens are 9 positions with end-of-text's, one past a chunk edge
P = 4
HEADS = [(0, 1), (1, 3)]
ENV, LENS, FRAMES = 192, [64, 128, 192, 128], [3000, 200, 3000, 3000]
PCM = np.stack([synth.synth_audio(s) for s in (7, 11, 13, 17)])


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from openhush_amd import engine
    assert hasattr(engine.lib(), "ohw_state_score")
    return engine


@pytest.fixture(scope="module")
def oracle():
    import os
    from oracle import oracle as o
    o.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    return o


@pytest.fixture(scope="module")
def ctxs(E):
    return {dt: E.Context.synthetic(MICRO.as_list(), 1234, 0, dt) for dt in (0, 1)}


def _tokens(ctx, counts=N_TEXT, seed=5):
    rng = np.random.default_rng(seed)
    return [[int(t) for t in rng.integers(0, ctx.tok.eot, size=n)] for n in counts]


def _state(E, ctx, windows=(0, 1, 2, 3), env=0, lens=None, invariant=False, packed=False):
    st = E.State(ctx, len(windows))
    st.set_batch_invariant(invariant)
    if env:
        st.set_audio_ctx(env)
    if lens is not None:
        st.set_window_ctx(lens)
    st.set_packed_encoder(packed)
    st.mel(PCM[list(windows)], [synth.CHUNK_SAMPLES] * len(windows), E.OHW_MEL_ZERO_TAIL, want=False)
    st.encode(len(windows))
    return st


def _bits(scores):
    return [s.tobytes() for s in scores]


def _launches(st):
    return st.counter("dec_gemm.total"), st.counter("xattn.total"), st.counter("token_score")


@pytest.mark.parametrize("dt", [0, 1])
def test_scores_match_the_oracle(E, oracle, ctxs, dt):
    ctx = ctxs[dt]
    tok, nv = ctx.tok, MICRO.n_vocab
    st = _state(E, ctx)
    st.set_score_buffers(2)
    p = ctx.default_params()
    toks = _tokens(ctx)
    enc = st.fetch("enc", 4)
    scores = st.score(toks, p=p)
    assert [len(s) for s in scores] == [0, 2, 5, 61]
    kept = st.fetch("score_logits", 4)                       # window 3: 4 + 60 + 1 positions in 9 chunks
    assert kept.shape == (72, nv)
    om = oracle.Model.synth(MICRO.as_list(), 1234)
    tol = 2 * TOL_LOGIT[dt]
    worst = dict(logit=0.0, top_logit=0.0, logprob_text=0.0, logprob_all=0.0, top_gap=0.0)
    for b in range(1, 4):
        seq = [tok.sot, tok.sot + 1 + p.lang_id, tok.translate if p.translate else tok.transcribe, tok.no_timestamps] + toks[b]
        s = oracle.State(om)
        s.set_encoder_output(enc[b])
        ref = np.asarray(s.decode(seq, 0, all_pos=True), np.float64)
        want = R.scores_from_logits(ref, P, toks[b], tok.eot, nv)
        for i, (g, w) in enumerate(zip(scores[b], want)):
            lt, la, _ = E.token_prob_host(g)
            errs = dict(logit=abs(float(g["logit"]) - w["logit"]), top_logit=abs(float(g["top_logit"]) - w["top_logit"]),
                        logprob_text=abs(float(lt) - (w["logit"] - w["lse_text"])), logprob_all=abs(float(la) - (w["logit"] - w["lse_all"])))
            row = ref[P - 1 + i]
            errs["top_gap"] = float(row[:tok.eot].max() - row[int(g["top_id"])])
            assert 0 <= int(g["top_id"]) < tok.eot
            for k, v in errs.items():
                worst[k] = max(worst[k], v)
                assert v < tol, (dt, b, i, k, v, tol)
    om.close()
    print(f"score vs oracle dt {dt}: worst " + ", ".join(f"{k} {v:.5f}" for k, v in worst.items()) + f" (tolerance {tol})")
    # the kept rows are the very words the kernel selected from
    for i, g in enumerate(scores[3]):
        target = toks[3][i] if i < 60 else tok.eot
        assert kept[P - 1 + i, target].view(np.uint32) == g["logit"].view(np.uint32), i
        assert kept[P - 1 + i, int(g["top_id"])].view(np.uint32) == g["top_logit"].view(np.uint32), i
        assert int(g["top_id"]) == int(np.argmax(kept[P - 1 + i, :tok.eot])), i
    # and the device's five words are the host rule's selections on those rows, its lse values inside the derived bound
    for i in (0, 4, 5, 60):
        target = toks[3][i] if i < 60 else tok.eot
        h = E.token_score_host(kept[P - 1 + i], tok.eot, target)
        g = scores[3][i]
        assert all(h[f].tobytes() == g[f].tobytes() for f in ("logit", "top_id", "top_logit")), i
        x = kept[P - 1 + i].astype(np.float64)
        assert abs(float(g["lse_text"]) - R.lse64(x[:tok.eot])) <= R.lse_bound(x[:tok.eot], nv) + abs(R.lse64(x[:tok.eot])) * R.U
        assert abs(float(g["lse_all"]) - R.lse64(x)) <= R.lse_bound(x, nv) + abs(R.lse64(x)) * R.U
    # releasing the buffers ends the fetch; the next call makes them again and gives the same bits
    st.set_score_buffers(0)
    with pytest.raises(E.WhisperError):
        st.fetch("score_logits", 4)
    assert _bits(st.score(toks, p=p)) == _bits(scores)
    st.close()


@pytest.mark.parametrize("dt", [0, 1])
def test_score_with_align_is_one_replay(E, ctxs, dt):
    ctx = ctxs[dt]
    st = _state(E, ctx, env=ENV, lens=LENS)
    p = ctx.default_params()
    toks = _tokens(ctx)
    only = st.score(toks, p=p)                                # no heads set: score-only needs none
    st.set_align_heads(HEADS)
    a0 = _launches(st)
    idx = st.align(toks, FRAMES, p)
    a1 = _launches(st)
    both, idx2 = st.score(toks, n_frames=FRAMES, p=p)
    a2 = _launches(st)
    assert _bits(both) == _bits(only)
    assert all(np.array_equal(x, y) for x, y in zip(idx, idx2)) and [len(x) for x in idx2] == [0, 2, 5, 61]
    chunks = (P + 60 + 1 + 7) // 8
    assert (a1[0] - a0[0], a1[1] - a0[1]) == (a2[0] - a1[0], a2[1] - a1[1]) and a1[0] > a0[0]
    assert a1[2] == a0[2] and a2[2] - a1[2] == chunks
    assert st.fetch("align_m", 4).shape == (61, 128)          # the fetches describe the combined call too
    assert _bits(st.score(toks, p=p)) == _bits(only)
    st.close()


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("packed", [False, True])
def test_a_window_alone_equals_the_window_in_the_batch(E, ctxs, dt, packed):
    ctx = ctxs[dt]
    p = ctx.default_params()
    toks = _tokens(ctx, counts=[9, 1, 4, 60])
    st = _state(E, ctx, env=ENV, lens=LENS, invariant=True, packed=packed)
    if packed:
        assert st.counter("enc_rows") == sum(LENS)
    batch = st.score(toks, p=p)
    part = st.score([toks[0], [], toks[2], toks[3]], p=p)      # a skipped window moves nothing
    assert len(part[1]) == 0 and _bits(part[0::2]) == _bits(batch[0::2]) and part[3].tobytes() == batch[3].tobytes()
    st.close()
    for b in range(4):
        one = _state(E, ctx, windows=(b,), env=LENS[b], invariant=True)
        alone = one.score([toks[b]], p=p)
        assert alone[0].tobytes() == batch[b].tobytes(), (b, alone[0][:2], batch[b][:2])
        one.close()


def test_refusals_launch_nothing(E, ctxs):
    ctx = ctxs[0]
    st = _state(E, ctx, env=ENV, lens=LENS)
    p = ctx.default_params()
    toks = _tokens(ctx)
    half = MICRO.n_text_ctx // 2
    good = st.score(toks, p=p)
    before = _launches(st)

    def refused(f, *words):
        with pytest.raises(E.WhisperError) as e:
            f()
        assert e.value.code == E.OHW_E_INVALID_ARG, (e.value.code, str(e.value))
        for w in words:
            assert w in str(e.value), (w, str(e.value))
        assert _launches(st) == before

    refused(lambda: st.score(toks, n_frames=FRAMES, p=p), "score", "no alignment heads")
    bad = [list(t) for t in toks]
    bad[2][1] = ctx.tok.eot
    refused(lambda: st.score(bad, p=p), "score: window 2", "token 1")
    bad[2][1] = -1
    refused(lambda: st.score(bad, p=p), "window 2", "token 1")
    refused(lambda: st.score([toks[0], [7] * (half + 1), toks[2], toks[3]], p=p), "window 1", str(half + 1))
    refused(lambda: st.score(toks[:3], p=p), "batch")
    st.set_align_heads(HEADS)
    refused(lambda: st.score(toks, n_frames=[3000, -1, 3000, 3000], p=p), "window 1", "n_frames")
    st.set_align_heads(None)
    st.set_window_lang([0, E.OHW_LANG_DETECT, 0, 0])
    refused(lambda: st.score(toks, p=p), "window 1", "language")
    st.set_window_lang(None)
    st.set_audio_ctx(128)
    refused(lambda: st.score(toks, p=p), "audio context")
    st.set_audio_ctx(ENV)
    refused(lambda: st.score(toks, p=p), "per-window contexts")
    st.set_window_ctx(LENS)
    L = E.lib()
    import ctypes as C
    one = np.zeros(4, np.int32)
    assert L.ohw_state_score(st.h, C.byref(p), None, 1, E._ip(one), 4, None, None, None) == E.OHW_E_INVALID_ARG
    assert "null" in E.last_error() and _launches(st) == before
    with pytest.raises(E.WhisperError):
        st.set_score_buffers(3)
    assert _bits(st.score(toks, p=p)) == _bits(good)          # n_text_ctx / 2 tokens fit, and nothing above left a trace
    assert len(st.score([toks[0], [7] * half, toks[2], toks[3]], p=p)[1]) == half + 1
    st.close()


def test_every_decode_mode_after_a_score_gives_a_fresh_states_bits(E, ctxs):
    ctx = ctxs[1]
    fresh = {}
    for name, fn in M.MODES.items():
        s = E.State(ctx, M.MAX_BATCH)
        fresh[name] = fn(E, ctx, s)
        s.close()
    st = E.State(ctx, M.MAX_BATCH)
    toks = _tokens(ctx, counts=[9, 0, 20])
    first = None
    for name, fn in M.MODES.items():
        st.mel(PCM[:3], None, E.OHW_MEL_ZERO_TAIL, want=False)
        st.encode(3)
        sc = _bits(st.score(toks))
        first = first or sc
        assert sc == first, name                               # and the score after every mode is the first score
        bad = M.same(fn(E, ctx, st), fresh[name])
        assert not bad, (name, bad[:4])
    st.close()
