"""Per-window language inside one decode batch (ohw_state_set_window_lang / _detect_window_lang / _window_lang) on the GPU.

The statement throughout is bit-equality: window b of a decode under a language table carries the tokens and the
log-probability bits of window b of a decode of the same state and audio with no table and p.lang_id = table[b].  The
prompt's language token is the only thing the table changes, and one decoder row never reads another's, so nothing weaker
is needed.  The languages 0, 17, 98 and 3 separate on the synthetic model (first-token log-probabilities -1.27, -1.30,
-1.68 and -2.31 on the CPU oracle for one window); the tests assert that separation on the GPU before they use it.

Detection: the synthetic model's [sot] step does not separate synth.synth_audio seeds (seeds 1 .. 30 all give language 91 on
the CPU oracle, margins 2.0 .. 3.3 logits), so the detection batch mixes two seeds with a silent and an attenuated clip, which
give language 84 (margins 0.56 and 0.82 on the oracle)."""
import numpy as np
import pytest

from openhush_amd import synth

from lang_rows import crafted_rows

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MICRO = synth.PRESETS["micro"]
LANGS = [0, 17, 98, 3]
N_MAX = 16
ENV = 256
LENS = [8, 63, 250, 256]


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from openhush_amd import engine
    assert hasattr(engine.lib(), "ohw_state_set_window_lang")
    return engine


@pytest.fixture(scope="module")
def ctxs(E):
    return {dt: E.Context.synthetic(MICRO.as_list(), 1234, 0, dt) for dt in (0, 1)}


def _pcm():
    short = np.zeros(synth.CHUNK_SAMPLES, np.float32)
    short[:48000] = synth.synth_audio(3, 48000)
    return (np.stack([synth.synth_audio(7), short, synth.synth_audio(11), synth.synth_audio(13)]),
            [synth.CHUNK_SAMPLES, 48000, synth.CHUNK_SAMPLES, synth.CHUNK_SAMPLES])


PCM, NS = _pcm()
# the detection batch: two seeds (language 91 on the oracle), silence and seed 7 at -60 dB (language 84)
DET = np.stack([synth.synth_audio(7), np.zeros(synth.CHUNK_SAMPLES, np.float32), synth.synth_audio(11), synth.synth_audio(7) * 1e-3])
DET_NS = [synth.CHUNK_SAMPLES] * 4


def _state(E, ctx, pcm=PCM, ns=NS, B=4, max_batch=None, lens=None, packed=False):
    st = E.State(ctx, max_batch or B)
    st.set_audio_ctx(ENV)
    if lens is not None:
        st.set_window_ctx(lens)
        st.set_packed_encoder(packed)
    st.mel(pcm[:B], ns[:B], E.OHW_MEL_ZERO_TAIL, want=False)
    st.encode(B)
    return st


def _params(ctx, lang=0):
    p = ctx.default_params()
    p.n_max = N_MAX
    p.lang_id = lang
    return p


def _same(x, y):
    return (x["tokens"] == y["tokens"] and np.array_equal(x["logprobs"], y["logprobs"]) and x["ended_by_eot"] == y["ended_by_eot"]
            and np.float32(x["no_speech_prob"]).tobytes() == np.float32(y["no_speech_prob"]).tobytes())


def _refused(E, f):
    with pytest.raises(E.WhisperError) as e:
        f()
    return e.value


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the kernel against its host definition
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset", ["micro", "micro-v3"])
def test_device_pick_equals_the_host_twin(E, preset):
    hp = synth.PRESETS[preset]
    ctx = E.Context.synthetic(hp.as_list(), 1234, 0, 1)
    assert ctx.tok.n_langs == hp.n_langs and hp.n_langs % 64 != 0
    st = E.State(ctx, 5)
    rows, want = crafted_rows(hp.n_vocab, hp.n_langs, ctx.tok.sot)
    ids, probs = st.dbg_lang_pick(rows)
    for r, row in enumerate(rows):
        hi, hprob = E.lang_pick_host(row, ctx.tok)
        err = float(np.abs(probs[r] - hprob).max())
        print(f"{preset} row {r}: device id {int(ids[r])} host id {hi} max abs probability err {err:.3g} (bound 1e-5)")
        assert int(ids[r]) == hi == want[r], (r, int(ids[r]), hi, want[r])
        assert err < 1e-5, (r, err)
    # a second call on fewer rows: nothing of the first call's table or rows is left behind
    ids2, probs2 = st.dbg_lang_pick(rows[3:])
    assert list(ids2) == want[3:] and np.array_equal(probs2, probs[3:])
    st.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. explicit languages
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [0, 1])
def test_explicit_languages_equal_the_uniform_runs(E, ctxs, dt):
    ctx = ctxs[dt]
    st = _state(E, ctx, max_batch=12)                # 12 rows: beam_search(K = 3) of 4 windows
    cap = ctx.hp.n_text_ctx
    u = np.random.default_rng(3).random((4, cap))
    active = [1, 1, 0, 1]
    uni = {}
    for L in LANGS:
        p = _params(ctx, L)
        uni[L] = (st.greedy_ex(4, p), st.sample_pass(4, 0.4, active, u, p), st.beam_search(4, 3, _params(ctx, L)))
    # not vacuous: for every window, the run at any other language of the table differs in a log-probability bit
    for b, L in enumerate(LANGS):
        for other in LANGS:
            if other != L:
                assert not np.array_equal(uni[L][0][b]["logprobs"], uni[other][0][b]["logprobs"]), (b, L, other)
    c0 = st.counter("step_captures"), st.counter("beam_captures")
    st.set_window_lang(LANGS)
    ids, probs = st.window_lang(4)
    assert list(ids) == LANGS and all(probs[b, L] == 1.0 and probs[b].sum() == 1.0 for b, L in enumerate(LANGS))
    p = _params(ctx, 55)                             # ignored while the table is set
    g = st.greedy_ex(4, p)
    s = st.sample_pass(4, 0.4, active, u, p)
    bm = st.beam_search(4, 3, p)
    for b, L in enumerate(LANGS):
        assert _same(g[b], uni[L][0][b]), ("greedy", b, L)
        assert len(g[b]["tokens"]) > 0
        if active[b]:
            assert _same(s[b], uni[L][1][b]) and len(s[b]["tokens"]) > 0, ("sample_pass", b, L)
        else:
            assert s[b]["tokens"] == []
        assert bm[b] == uni[L][2][b], ("beam", b, L)
    toks, slp = st.greedy(4, p)                       # ohw_greedy goes through the same loop
    assert toks == [x["tokens"] for x in g]
    # the prompt is outside the replayed graphs: other languages, no new capture
    assert (st.counter("step_captures"), st.counter("beam_captures")) == c0
    st.set_window_lang(LANGS[::-1])
    g2 = st.greedy_ex(4, p)
    assert all(_same(g2[b], uni[L][0][b]) for b, L in enumerate(LANGS[::-1]))
    assert (st.counter("step_captures"), st.counter("beam_captures")) == c0
    # clearing the table restores the bits of a run that never had one
    st.set_window_lang(None)
    back = st.greedy_ex(4, _params(ctx, 17))
    assert all(_same(back[b], uni[17][0][b]) for b in range(4))
    st.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. detection
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [0, 1])
def test_detection_on_the_device_equals_the_host_path(E, ctxs, dt):
    ctx = ctxs[dt]
    st = _state(E, ctx, DET, DET_NS)
    hid, hprob = st.detect_language(4)
    print(f"dtype {dt}: host-path ids {list(hid)}")
    assert len(set(int(x) for x in hid)) >= 2, list(hid)          # the clips were chosen to separate (module docstring)
    st.set_window_lang([E.OHW_LANG_DETECT] * 4)
    ids, probs = st.window_lang(4)
    assert list(ids) == [-1] * 4 and not probs.any()
    st.detect_window_lang(4)
    ids, probs = st.window_lang(4)
    err = float(np.abs(probs - hprob).max())
    print(f"dtype {dt}: device ids {list(ids)} max abs probability err {err:.3g} (bound 1e-5)")
    assert list(ids) == list(hid)
    assert err < 1e-5
    g = st.greedy_ex(4, _params(ctx, 0))
    st.detect_window_lang(4)                                       # nothing pending: a no-op
    assert list(st.window_lang(4)[0]) == list(hid)
    # explicit entries are kept, pending ones resolved
    st.set_window_lang([-1, 5, -1, 9])
    st.detect_window_lang(4)
    ids2, probs2 = st.window_lang(4)
    assert list(ids2) == [int(hid[0]), 5, int(hid[2]), 9]
    assert probs2[1, 5] == 1.0 and probs2[3, 9] == 1.0 and np.array_equal(probs2[0], probs[0]) and np.array_equal(probs2[2], probs[2])
    gm = st.greedy_ex(4, _params(ctx, 0))
    st.set_window_lang(None)
    uni = {L: st.greedy_ex(4, _params(ctx, L)) for L in sorted(set(int(x) for x in hid) | {5, 9})}
    for b in range(4):
        assert _same(g[b], uni[int(hid[b])][b]), b
        assert _same(gm[b], uni[[int(hid[0]), 5, int(hid[2]), 9][b]][b]), b
    st.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. lengths and packing
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [0, 1])
def test_mixed_languages_under_window_ctx_and_the_packed_encoder(E, ctxs, dt):
    ctx = ctxs[dt]
    st = _state(E, ctx, lens=LENS, packed=True)
    st.set_batch_invariant(True)
    st.set_window_lang([LANGS[0], E.OHW_LANG_DETECT, LANGS[2], E.OHW_LANG_DETECT])
    st.detect_window_lang(4)
    ids, _ = st.window_lang(4)
    table = [int(x) for x in ids]
    assert table[0] == LANGS[0] and table[2] == LANGS[2]
    # the detected windows carry ids of their own, not a neighbour's explicit one
    assert all(0 <= table[b] < ctx.tok.n_langs and table[b] not in (LANGS[0], LANGS[2]) for b in (1, 3)), table
    g = st.greedy_ex(4, _params(ctx, 0))
    for b, n in enumerate(LENS):
        one = E.State(ctx, 1)
        one.set_audio_ctx(n)
        one.set_batch_invariant(True)
        one.mel(PCM[b:b + 1], NS[b:b + 1], E.OHW_MEL_ZERO_TAIL, want=False)
        one.encode(1)
        if b in (1, 3):
            assert int(one.detect_language(1)[0][0]) == table[b], (b, table)
        ref = one.greedy_ex(1, _params(ctx, table[b]))[0]
        assert _same(g[b], ref), (b, n, table[b])
        one.close()
    st.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. contracts
# ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_life_of_an_entry(E, ctxs):
    ctx = ctxs[1]
    nl = ctx.tok.n_langs
    st = _state(E, ctx, DET, DET_NS, B=3, max_batch=6)         # 6 rows: beam_search(K = 2) of 3 windows
    p = _params(ctx, 0)
    base = st.greedy_ex(3, p)
    assert _refused(E, lambda: st.set_window_lang([0, nl, 1])).code == E.OHW_E_INVALID_ARG
    assert _refused(E, lambda: st.set_window_lang([0, -2, 1])).code == E.OHW_E_INVALID_ARG
    assert _refused(E, lambda: st.set_window_lang([0] * 7)).code == E.OHW_E_INVALID_ARG           # more than max_batch
    assert all(_same(x, y) for x, y in zip(st.greedy_ex(3, p), base))                             # a refused call sets nothing
    # batch mismatch at decode
    st.set_window_lang([0, 1])
    for f in (lambda: st.greedy_ex(3, p), lambda: st.detect_window_lang(3), lambda: st.beam_search(3, 2, p),
              lambda: st.sample_pass(3, 0.4, [1, 1, 1], np.zeros((3, ctx.hp.n_text_ctx)), p)):
        assert _refused(E, f).code == E.OHW_E_INVALID_ARG
    # a pending entry never decodes as English
    st.set_window_lang([3, E.OHW_LANG_DETECT, 3])
    err = _refused(E, lambda: st.greedy_ex(3, p))
    assert err.code == E.OHW_E_INVALID_ARG and "detect" in str(err)
    err = _refused(E, lambda: st.beam_search(3, 2, p))
    assert err.code == E.OHW_E_INVALID_ARG and "detect" in str(err)
    st.detect_window_lang(3)
    first = st.greedy_ex(3, p)
    detected = int(st.window_lang(3)[0][1])
    # a new encode: the detected entry waits again, the explicit ones would decode
    st.mel(DET[:3], DET_NS[:3], E.OHW_MEL_ZERO_TAIL, want=False)
    st.encode(3)
    assert list(st.window_lang(3)[0]) == [3, -1, 3]
    assert _refused(E, lambda: st.greedy_ex(3, p)).code == E.OHW_E_INVALID_ARG
    st.set_audio_ctx(ENV)                                     # does not touch the table
    assert list(st.window_lang(3)[0]) == [3, -1, 3]
    st.detect_window_lang(3)
    assert int(st.window_lang(3)[0][1]) == detected
    assert all(_same(x, y) for x, y in zip(st.greedy_ex(3, p), first))
    st.set_window_lang([3, 4, 3])                             # all explicit: a new encode changes nothing
    st.mel(DET[:3], DET_NS[:3], E.OHW_MEL_ZERO_TAIL, want=False)
    st.encode(3)
    assert list(st.window_lang(3)[0]) == [3, 4, 3]
    st.greedy_ex(3, p)
    st.set_window_lang(None)
    assert all(_same(x, y) for x, y in zip(st.greedy_ex(3, p), base))
    assert _refused(E, lambda: st.window_lang(3)).code == E.OHW_E_INVALID_ARG
    st.close()
    # an English-only model has no language token
    hl = MICRO.as_list()
    hl[0] = 51864
    en = E.Context.synthetic(hl, 1234, 0, 1)
    s2 = E.State(en, 2)
    assert _refused(E, lambda: s2.set_window_lang([0, 0])).code == E.OHW_E_INVALID_ARG
    s2.close()
