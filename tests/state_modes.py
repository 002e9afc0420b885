"""The decode modes one ohw_state is switched between, for tests/test_gpu_state_reuse.py: a table MODES of name ->
run(E, ctx, st) -> result, a bit-exact comparison `same`, and the interleaved order `schedule` the GPU test walks.  Plain
Python: importing this module needs no GPU and no library.

Every mode obeys four rules, so that any mode may follow any other on one state:
  1. it makes all of its own inputs from fixed seeds (audio from synth.synth_audio, draws from numpy generators, phrase lists);
  2. it runs its own mel and encode and depends on no earlier call;
  3. it sets every setting it needs and, before it returns, puts back every setting it touched (tables to None, rules off,
     audio context 0, packed / invariant / persistent off, prefill chunk 8) - putting them back is part of what is tested;
  4. it returns a flat dict: tokens and flags as lists of ints, every float (logits, log-probabilities, sums, no-speech
     probabilities, command_list_logprob) as its raw uint32 words, so equality is bit equality and a NaN equals itself.

Micro model, max_batch 15, n_max <= 12.  Where a decode carries the bias of tests/test_gpu_persist.py (timestamps + 6, end of
text + 27) the rows of a batch end at different steps.  The modes' graph keys differ from each other (rows, n_max, flags), so a
walk over all of them overflows the step cache (8 keys) and, from a beam mode, the beam cache (4 keys)."""
import functools

import numpy as np

from openhush_amd import synth

MAX_BATCH = 15
TOP = [47018, 17019, 20198, 8911, 11308]            # text tokens the procedural model favours (tests/test_gpu_commands.py)
COMMANDS = [[47018, 17019], [47018, 17019, 20198], [8911], [11308, 8911, 47018, 17019, 20198, 8911], [20198, 11308]]
ALIGN_HEADS = [(0, 1), (1, 3)]                      # two heads in two layers
LANG_DETECT = -1                                    # OHW_LANG_DETECT


# ---- inputs ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _audio(seed: int) -> np.ndarray:
    a = synth.synth_audio(seed)
    a.setflags(write=False)
    return a


def _pcm(seeds) -> np.ndarray:
    return np.stack([_audio(s) for s in seeds])


def _encode(E, st, seeds):
    st.mel(_pcm(seeds), None, E.OHW_MEL_ZERO_TAIL, want=False)
    st.encode(len(seeds))


def _bias(ctx, ts_b=6.0, eot_b=27.0) -> np.ndarray:
    b = np.zeros(ctx.hp.n_vocab, np.float32)
    b[ctx.tok.timestamp_begin:] = ts_b
    b[ctx.tok.eot] = eot_b
    return b


def _params(ctx, n_max: int, **kw):
    p = ctx.default_params()
    p.n_max = n_max
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _uniforms(seed: int, shape) -> np.ndarray:
    return np.random.default_rng(seed).random(shape)


def _contexts(ctx, lens, seed: int):
    rng = np.random.default_rng(seed)
    return [[int(t) for t in rng.integers(0, ctx.tok.eot, size=n)] for n in lens]


# ---- results ---------------------------------------------------------------------------------------------------------------
def bits(x) -> np.ndarray:
    """float32 values -> their uint32 words (a copy)"""
    return np.ascontiguousarray(np.atleast_1d(np.asarray(x, dtype=np.float32))).view(np.uint32).copy()


def _put_rows(out: dict, name: str, rows):
    """the dicts of greedy_ex / sample_pass / sample_pass_n / beam_search / beam_search_ex, flattened under `name`"""
    for i, r in enumerate(rows):
        out[f"{name}.{i}.tokens"] = [int(t) for t in r["tokens"]]
        out[f"{name}.{i}.sum_logprob"] = bits(r["sum_logprob"])
        if "logprobs" in r:
            out[f"{name}.{i}.logprobs"] = bits(r["logprobs"])
            out[f"{name}.{i}.ended_by_eot"] = [int(r["ended_by_eot"])]
            out[f"{name}.{i}.no_speech_prob"] = bits(r["no_speech_prob"])
        if "n_finished" in r:
            out[f"{name}.{i}.n_finished"] = [int(r["n_finished"])]


def _flat(v) -> np.ndarray:
    if isinstance(v, (list, tuple)) and len(v) == 0:        # an inactive row's tokens: numpy would make an empty list float64
        return np.zeros(0, np.int64)
    return np.asarray(v).reshape(-1)


def same(a: dict, b: dict) -> list:
    """the keys in which two results differ: a key only one of them has, another length, another int, another word"""
    bad = []
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            bad.append(k)
            continue
        x, y = _flat(a[k]), _flat(b[k])
        if x.dtype.kind not in "iu" or y.dtype.kind not in "iu":
            raise TypeError(f"{k}: results hold ints and uint32 words only, not {x.dtype} / {y.dtype}")
        if x.shape != y.shape or not np.array_equal(x, y):
            bad.append(k)
    return bad


def first_difference(a: dict, b: dict, key: str) -> int:
    """the first index at which a[key] and b[key] differ (the shorter length when one is a prefix of the other; -1: a missing key)"""
    if key not in a or key not in b:
        return -1
    x, y = _flat(a[key]), _flat(b[key])
    n = min(x.size, y.size)
    d = np.nonzero(x[:n] != y[:n])[0]
    return int(d[0]) if d.size else n


def schedule(a: str, names) -> list:
    """[a, b0, a, b1, a, ..., b_last, a]: every (a, b) and every (b, a) is a pair of neighbours, b == a included"""
    order = [a]
    for b in names:
        order += [b, a]
    return order


def walk(run, order, fresh, compare=None) -> list:
    """run(name) for every name of `order` on one state; -> one (previous mode, this mode, differing keys, first differing
    index of the first such key) per step whose result is not fresh[name] under `compare` (default: same)"""
    failures, prev = [], None
    for name in order:
        got = run(name)
        bad = (compare or same)(got, fresh[name])
        if bad:
            failures.append((prev, name, bad, first_difference(got, fresh[name], bad[0])))
        prev = name
    return failures


# ---- the modes -------------------------------------------------------------------------------------------------------------
MODES = {}


def mode(fn):
    MODES[fn.__name__] = fn
    return fn


@mode
def logits3(E, ctx, st):
    """decode: a 3-token prompt on 3 windows, then 4 single-token steps with ragged n_past (row 1 is rewound by two positions);
    raw logits.  Restores nothing: it touches no setting."""
    tok = ctx.tok
    _encode(E, st, (40, 41, 42))
    prompt = np.tile(np.asarray([tok.sot, tok.sot + 1, tok.transcribe], np.int32), (3, 1))
    lg = st.decode(prompt, [0, 0, 0])
    out = {"prompt": bits(lg)}
    for i, n_past in enumerate(([3, 3, 3], [4, 4, 4], [5, 3, 5], [6, 4, 6])):
        feed = lg.argmax(axis=1).astype(np.int32)[:, None]
        out[f"step{i}.feed"] = [int(t) for t in feed[:, 0]]
        lg = st.decode(feed, n_past)
        out[f"step{i}"] = bits(lg)
    return out


@mode
def greedy3(E, ctx, st):
    """greedy_ex on 3 windows, no bias.  Restores nothing: it touches no setting."""
    _encode(E, st, (3, 11, 7))
    out = {}
    _put_rows(out, "greedy", st.greedy_ex(3, _params(ctx, 12)))
    return out


@mode
def greedy1(E, ctx, st):
    """greedy_ex on 1 window: fewer rows than any predecessor.  Restores nothing: it touches no setting."""
    _encode(E, st, (5,))
    out = {}
    _put_rows(out, "greedy", st.greedy_ex(1, _params(ctx, 11)))
    return out


@mode
def greedy_bias(E, ctx, st):
    """set_logit_bias, greedy_ex on 3 windows.  Restores: the logit bias (cleared)."""
    _encode(E, st, (7, 3, 11))
    st.set_logit_bias(_bias(ctx))
    out = {}
    _put_rows(out, "greedy", st.greedy_ex(3, _params(ctx, 10)))
    st.set_logit_bias(None)
    return out


def leaky_greedy_bias(E, ctx, st):
    """greedy_bias without its last line: the bias stays on the state.  Not in MODES; the GPU test uses it to show that the
    walk sees a setting that leaks.  Restores nothing, on purpose."""
    _encode(E, st, (7, 3, 11))
    st.set_logit_bias(_bias(ctx))
    out = {}
    _put_rows(out, "greedy", st.greedy_ex(3, _params(ctx, 10)))
    return out


@mode
def temp(E, ctx, st):
    """sample_pass at T = 0.6 on 3 windows, window 1 inactive, under the bias.  Restores: the logit bias (cleared)."""
    _encode(E, st, (11, 7, 3))
    st.set_logit_bias(_bias(ctx))
    u = _uniforms(31, (3, ctx.hp.n_text_ctx))
    out = {}
    _put_rows(out, "pass", st.sample_pass(3, 0.6, [1, 0, 1], u, _params(ctx, 12)))
    st.set_logit_bias(None)
    return out


@mode
def bestof3(E, ctx, st):
    """sample_pass_n, best_of 3 on 2 windows at T = 0.6, then a second pass at T = 0.8 with window 1 inactive, under the bias.
    Restores: the logit bias (cleared)."""
    _encode(E, st, (7, 3))
    st.set_logit_bias(_bias(ctx))
    cap = ctx.hp.n_text_ctx
    p = _params(ctx, 12)
    out = {}
    _put_rows(out, "pass0", st.sample_pass_n(2, 3, 0.6, [1, 1], _uniforms(32, (2, 3, cap)), p))
    _put_rows(out, "pass1", st.sample_pass_n(2, 3, 0.8, [1, 0], _uniforms(33, (2, 3, cap)), p))
    st.set_logit_bias(None)
    return out


@mode
def beam5(E, ctx, st):
    """beam_search_ex, K = 5 on 2 windows, under the bias.  Restores: the logit bias (cleared)."""
    _encode(E, st, (3, 11))
    st.set_logit_bias(_bias(ctx))
    out = {}
    _put_rows(out, "beam", st.beam_search_ex(2, 5, _params(ctx, 10)))
    st.set_logit_bias(None)
    return out


@mode
def beam2(E, ctx, st):
    """beam_search, K = 2 on 3 windows (the other buffer parity, another graph key), under the bias.  Restores: the logit bias
    (cleared)."""
    _encode(E, st, (11, 3, 7))
    st.set_logit_bias(_bias(ctx))
    out = {}
    _put_rows(out, "beam", st.beam_search(3, 2, _params(ctx, 9)))
    st.set_logit_bias(None)
    return out


@mode
def prompt8(E, ctx, st):
    """set_window_prompt with contexts of 5, 0 and 11 tokens, prefill in chunks of 8, greedy_ex.  Restores: the prompt table
    (None); the prefill chunk is set to 8, the default, and stays there."""
    _encode(E, st, (13, 7, 3))
    st.set_prefill_chunk(8)
    st.set_window_prompt(_contexts(ctx, (5, 0, 11), 6))
    st.prefill(3)
    out = {"prompt_len": [st.window_prompt_len(b) for b in range(3)]}
    _put_rows(out, "greedy", st.greedy_ex(3, _params(ctx, 9)))
    st.set_window_prompt(None)
    return out


@mode
def prompt16_beam(E, ctx, st):
    """set_window_prompt with contexts of 17, 0 and 9 tokens, prefill in chunks of 16, greedy_ex, then beam_search K = 3 under
    the same table (the table moves the prefix: prefix_stride = K), under the bias.  Restores: the prompt table (None), the
    prefill chunk (8), the logit bias (cleared)."""
    _encode(E, st, (3, 13, 11))
    st.set_logit_bias(_bias(ctx))
    st.set_prefill_chunk(16)
    st.set_window_prompt(_contexts(ctx, (17, 0, 9), 8))
    st.prefill(3)
    p = _params(ctx, 8)
    out = {"prompt_len": [st.window_prompt_len(b) for b in range(3)]}
    _put_rows(out, "greedy", st.greedy_ex(3, p))
    _put_rows(out, "beam", st.beam_search(3, 3, p))
    st.set_window_prompt(None)
    st.set_prefill_chunk(8)
    st.set_logit_bias(None)
    return out


@mode
def ctx_mixed(E, ctx, st):
    """set_audio_ctx envelope 256, set_window_ctx 64 / 250 / 256, packed encoder on, greedy_ex.  Restores: the packed encoder
    (off), the window contexts (None), the audio context (0)."""
    st.set_audio_ctx(256)
    st.set_window_ctx([64, 250, 256])
    st.set_packed_encoder(True)
    _encode(E, st, (7, 11, 13))
    out = {"window_ctx": [st.window_ctx(b) for b in range(3)]}
    _put_rows(out, "greedy", st.greedy_ex(3, _params(ctx, 12)))
    st.set_packed_encoder(False)
    st.set_window_ctx(None)
    st.set_audio_ctx(0)
    return out


@mode
def lang_detect(E, ctx, st):
    """set_window_lang with one explicit id and three pending entries on 4 windows (two seeds, silence, an attenuated clip),
    detect_window_lang, greedy_ex.  Restores: the language table (None)."""
    pcm = np.stack([_audio(7), np.zeros(synth.CHUNK_SAMPLES, np.float32), _audio(11), _audio(7) * np.float32(1e-3)])
    st.mel(pcm, None, E.OHW_MEL_ZERO_TAIL, want=False)
    st.encode(4)
    st.set_window_lang([17, LANG_DETECT, LANG_DETECT, LANG_DETECT])
    st.detect_window_lang(4)
    ids, probs = st.window_lang(4)
    out = {"lang.ids": [int(i) for i in ids], "lang.probs": bits(probs)}
    _put_rows(out, "greedy", st.greedy_ex(4, _params(ctx, 10)))
    st.set_window_lang(None)
    return out


@mode
def rules(E, ctx, st):
    """hot phrases, the repetition rule (penalty 1.3, no-repeat 3-grams) and a command list at penalty 100; greedy_ex on 3
    windows, then beam_search K = 2; command_list_logprob after each, asked for 4 entries (the fourth window never decodes: its
    entry is the NaN the buffer starts as).  Restores: the phrase table (None), the repetition rule (off), the command list
    (None)."""
    _encode(E, st, (7, 3, 11))
    st.set_phrase_table([TOP[:2], [TOP[3]], [TOP[2], TOP[4], TOP[0]]], [2.0, 1.5, 3.0])
    st.set_repeat_rule(1.3, 3)
    st.set_command_table(COMMANDS, 100.0)
    p = _params(ctx, 11)
    out = {}
    _put_rows(out, "greedy", st.greedy_ex(3, p))
    out["greedy.list_logprob"] = bits(st.command_list_logprob(4))
    _put_rows(out, "beam", st.beam_search(3, 2, p))
    out["beam.list_logprob"] = bits(st.command_list_logprob(4))
    st.set_phrase_table(None)
    st.set_repeat_rule(1.0, 0)
    st.set_command_table(None)
    return out


@mode
def align(E, ctx, st):
    """set_align_heads (two heads in two layers) under an envelope of 192 with window contexts 64 / 128 / 192, greedy_ex of 7
    forced text tokens, align on those tokens.  Restores: the alignment heads (None), the window contexts (None), the audio
    context (0)."""
    st.set_audio_ctx(192)
    st.set_window_ctx([64, 128, 192])
    _encode(E, st, (7, 11, 13))
    p = _params(ctx, 12, no_timestamps=1, force_len=7)
    g = st.greedy_ex(3, p)
    out = {}
    _put_rows(out, "greedy", g)
    st.set_align_heads(ALIGN_HEADS)
    idx = st.align([r["tokens"] for r in g], [3000, 200, 3000], p)
    for b, ix in enumerate(idx):
        out[f"align.{b}"] = [int(i) for i in ix]
    st.set_align_heads(None)
    st.set_window_ctx(None)
    st.set_audio_ctx(0)
    return out


@mode
def invariant(E, ctx, st):
    """set_batch_invariant(True), greedy_ex on 3 windows.  Restores: batch invariance (off)."""
    st.set_batch_invariant(True)
    _encode(E, st, (11, 13, 3))
    out = {}
    _put_rows(out, "greedy", st.greedy_ex(3, _params(ctx, 12)))
    st.set_batch_invariant(False)
    return out


@mode
def persist(E, ctx, st):
    """set_persistent(True); two single-token decode steps (raw logits of the one-launch step), then greedy_ex on 3 windows and
    beam_search K = 2 under the bias.  persist_launches must have grown: the counter is kept on the host, so a replayed graph
    adds nothing to it and the two decode steps, which are never captured, are what makes it grow on every run.  Restores: the
    persistent step (off), the logit bias (cleared)."""
    tok = ctx.tok
    st.set_persistent(True)
    _encode(E, st, (3, 11, 7))
    launches = st.counter("persist_launches")
    lg = st.decode(np.tile(np.asarray([tok.sot, tok.sot + 1, tok.transcribe], np.int32), (3, 1)), [0, 0, 0])
    out = {}
    for i in range(2):
        lg = st.decode(lg.argmax(axis=1).astype(np.int32)[:, None], [3 + i] * 3)
        out[f"step{i}"] = bits(lg)
    assert st.counter("persist_launches") == launches + 2, "the single-token steps did not take the persistent path"
    st.set_logit_bias(_bias(ctx))
    p = _params(ctx, 12)
    _put_rows(out, "greedy", st.greedy_ex(3, p))
    _put_rows(out, "beam", st.beam_search(3, 2, p))
    assert st.counter("persist_launches") > launches, "the persistent step never ran"
    st.set_logit_bias(None)
    st.set_persistent(False)
    return out
