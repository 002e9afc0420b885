"""The replayed-iteration graph caches of the three device decode loops (greedy / sample_pass, sample_pass_n, beam search), micro
model, f16, 2 windows, n_max 8 .. 17.

What is pinned: a first call of a key captures exactly once and a repeat never; each cache holds its capacity (step 8, group 4,
beam 4 pairs) and an evicted key captures again and gives what it first gave; a temperature pass is a key of its own; a state
made under OHW_GRAPHS=0 gives the same bits through the launched kernels and keeps every counter at 0; OHW_GRAPH_MAX_BATCH
bounds the single-row loop alone; and the entries' argument errors carry their texts."""
import numpy as np
import pytest

from openhush_amd import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

T_PASS = 0.6
COUNTERS = ("step_captures", "step_graphs", "group_graphs", "beam_captures", "beam_graphs")


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from openhush_amd import engine
    engine.lib()
    return engine


@pytest.fixture(scope="module")
def ctx(E, tmp_models):
    return E.Context.from_file(tmp_models("micro"), 0, E.OHW_DTYPE_F16)


@pytest.fixture(scope="module")
def pcm():
    return np.stack([synth.synth_audio(s) for s in (7, 3)])


def _state(E, ctx, rows):
    st = E.State(ctx, rows)
    b = np.zeros(ctx.hp.n_vocab, np.float32)          # timestamps and end-of-text compete: rows end at different steps
    b[ctx.tok.timestamp_begin:] = 6.0
    b[ctx.tok.eot] = 27.0
    st.set_logit_bias(b)
    return st


def _encode(E, st, pcm, W):
    st.mel(pcm[:W], None, E.OHW_MEL_ZERO_TAIL, want=False)
    st.encode(W)


def _params(ctx, n_max):
    p = ctx.default_params()
    p.n_max = n_max
    return p


def _uniforms(E, ctx, W, N):
    cap = ctx.hp.n_text_ctx
    return np.stack([np.stack([E.HostRng(j).uniforms(cap) for j in range(N)]) for _ in range(W)])


def _same(a, b):
    return (a["tokens"] == b["tokens"] and a["ended_by_eot"] == b["ended_by_eot"]
            and np.array_equal(a["logprobs"].view(np.uint32), b["logprobs"].view(np.uint32))
            and np.float32(a["no_speech_prob"]).view(np.uint32) == np.float32(b["no_speech_prob"]).view(np.uint32))


def _all_same(a, b):
    return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))


def _beam_same(a, b):
    return len(a) == len(b) and all(
        _same(x, y) and x["n_finished"] == y["n_finished"]
        and np.float32(x["sum_logprob"]).view(np.uint32) == np.float32(y["sum_logprob"]).view(np.uint32) for x, y in zip(a, b))


def test_step_cache_captures_once_per_key_holds_eight_and_recaptures_the_evicted(E, ctx, pcm):
    W = 2
    st = _state(E, ctx, W)
    _encode(E, st, pcm, W)
    first = {}
    for n_max in range(8, 18):                        # ten keys: n_max is a sampler parameter
        c0 = st.counter("step_captures")
        first[n_max] = st.greedy_ex(W, _params(ctx, n_max))
        assert st.counter("step_captures") == c0 + 1, n_max
        again = st.greedy_ex(W, _params(ctx, n_max))
        assert st.counter("step_captures") == c0 + 1, n_max
        assert [r["tokens"] for r in again] == [r["tokens"] for r in first[n_max]], n_max
    assert st.counter("step_graphs") == 8
    c0 = st.counter("step_captures")
    assert _all_same(st.greedy_ex(W, _params(ctx, 8)), first[8])             # evicted: captured again, the same result
    assert st.counter("step_captures") == c0 + 1 and st.counter("step_graphs") == 8
    assert _all_same(st.greedy_ex(W, _params(ctx, 17)), first[17])           # the newest key is still held
    assert st.counter("step_captures") == c0 + 1
    # a temperature pass with a cached greedy key's parameters is a key of its own
    u = _uniforms(E, ctx, W, 1)[:, 0, :].copy()
    t1 = st.sample_pass(W, T_PASS, [1] * W, u, _params(ctx, 17))
    assert st.counter("step_captures") == c0 + 2
    assert _all_same(st.sample_pass(W, T_PASS, [1] * W, u, _params(ctx, 17)), t1)
    assert st.counter("step_captures") == c0 + 2 and st.counter("step_graphs") == 8
    assert st.counter("group_graphs") == 0 and st.counter("beam_graphs") == 0 and st.counter("beam_captures") == 0


def test_group_cache_captures_once_per_key_holds_four_and_recaptures_the_evicted(E, ctx, pcm):
    st = _state(E, ctx, 6)
    _encode(E, st, pcm, 2)
    st.greedy_ex(2, _params(ctx, 12))
    assert st.counter("step_graphs") == 1 and st.counter("step_captures") == 1
    keys = [(2, 2, 12), (2, 3, 12), (1, 2, 12), (1, 3, 12), (1, 5, 12), (1, 5, 13)]
    first = {}
    enc = 2
    for W, N, n_max in keys:
        if W != enc:
            _encode(E, st, pcm, W)
            enc = W
        u = _uniforms(E, ctx, W, N)
        c0 = st.counter("step_captures")
        first[(W, N, n_max)] = st.sample_pass_n(W, N, T_PASS, [1] * W, u, _params(ctx, n_max))
        assert st.counter("step_captures") == c0 + 1, (W, N, n_max)
        again = st.sample_pass_n(W, N, T_PASS, [1] * W, u, _params(ctx, n_max))
        assert st.counter("step_captures") == c0 + 1, (W, N, n_max)
        assert _all_same(again, first[(W, N, n_max)]), (W, N, n_max)
    assert st.counter("group_graphs") == 4
    _encode(E, st, pcm, 2)
    c0 = st.counter("step_captures")
    assert _all_same(st.sample_pass_n(2, 2, T_PASS, [1, 1], _uniforms(E, ctx, 2, 2), _params(ctx, 12)), first[(2, 2, 12)])
    assert st.counter("step_captures") == c0 + 1 and st.counter("group_graphs") == 4
    assert st.counter("step_graphs") == 1             # the group passes never touch the single-row cache
    assert st.counter("beam_graphs") == 0 and st.counter("beam_captures") == 0


def test_graphs_off_gives_the_bits_of_graphs_on_in_all_three_loops(E, ctx, pcm, monkeypatch):
    W = 2
    on = _state(E, ctx, 6)
    monkeypatch.setenv("OHW_GRAPHS", "0")             # the state reads it when it is made
    off = _state(E, ctx, 6)
    monkeypatch.delenv("OHW_GRAPHS")
    p = _params(ctx, 16)
    u1, u3 = _uniforms(E, ctx, W, 1)[:, 0, :].copy(), _uniforms(E, ctx, W, 3)
    got = {}
    for name, st in (("on", on), ("off", off)):
        _encode(E, st, pcm, W)
        g = st.greedy_ex(W, p)
        g_steps = st.timings().decode_steps
        s1 = st.sample_pass(W, T_PASS, [1] * W, u1, p)
        s3 = st.sample_pass_n(W, 3, T_PASS, [1] * W, u3, p)
        b = st.beam_search_ex(W, 3, p)
        got[name] = (g, g_steps, s1, s3, b, st.timings().decode_steps)
    a, z = got["on"], got["off"]
    assert _all_same(a[0], z[0]) and _all_same(a[2], z[2]) and _all_same(a[3], z[3]) and _beam_same(a[4], z[4])
    assert a[1] == z[1] and a[5] == z[5] and 1 <= a[1] <= 16 and 1 <= a[5] <= 16
    assert len({tuple(r["tokens"]) for r in a[3]}) > 1
    assert [on.counter(c) for c in COUNTERS] == [3, 2, 1, 1, 1]      # a group capture counts in step_captures
    assert [off.counter(c) for c in COUNTERS] == [0, 0, 0, 0, 0]


def test_graph_max_batch_bounds_the_single_row_loop_alone(E, ctx, pcm, monkeypatch):
    monkeypatch.setenv("OHW_GRAPH_MAX_BATCH", "2")    # read when the state is made: graphs for batches below 2
    st = _state(E, ctx, 4)
    monkeypatch.delenv("OHW_GRAPH_MAX_BATCH")
    p = _params(ctx, 12)
    _encode(E, st, pcm, 2)
    st.greedy_ex(2, p)
    assert st.counter("step_captures") == 0 and st.counter("step_graphs") == 0
    st.sample_pass_n(2, 2, T_PASS, [1, 1], _uniforms(E, ctx, 2, 2), p)
    assert st.counter("step_captures") == 1 and st.counter("group_graphs") == 1
    st.beam_search(2, 2, p)
    assert st.counter("beam_captures") == 1 and st.counter("beam_graphs") == 1
    _encode(E, st, pcm, 1)
    st.greedy_ex(1, p)
    assert st.counter("step_captures") == 2 and st.counter("step_graphs") == 1


def test_argument_errors_keep_their_texts(E, ctx, pcm):
    W, N = 2, 3
    p = _params(ctx, 12)
    u1, u3 = _uniforms(E, ctx, W, 1)[:, 0, :].copy(), _uniforms(E, ctx, W, N)

    def message(call):
        with pytest.raises(E.WhisperError) as e:
            call()
        assert e.value.code == E.OHW_E_INVALID_ARG
        return str(e.value)

    st = _state(E, ctx, W * N)                        # nothing encoded yet
    assert message(lambda: st.greedy_ex(W, p)) == "greedy: batch must equal the batch of the last ohw_encode"
    assert message(lambda: st.sample_pass(W, T_PASS, [1] * W, u1, p)) == "sample_pass: batch must equal the batch of the last ohw_encode"
    assert message(lambda: st.sample_pass_n(W, N, T_PASS, [1] * W, u3, p)) == "sample_pass_n: n_windows must equal the batch of the last ohw_encode"
    assert message(lambda: st.beam_search(W, N, p)) == "beam search: n_windows must equal the batch of the last ohw_encode"
    assert message(lambda: st.beam_search_ex(W, N, p)) == "beam search: n_windows must equal the batch of the last ohw_encode"
    small = _state(E, ctx, W * N - 1)                 # one decoder row short of W * N
    _encode(E, small, pcm, W)
    assert message(lambda: small.sample_pass_n(W, N, T_PASS, [1] * W, u3, p)) == "sample_pass_n: the state needs max_batch >= n_windows * best_of decoder rows"
    assert message(lambda: small.beam_search(W, N, p)) == "beam search: the state needs max_batch >= n_windows * beam_size decoder rows"
    assert message(lambda: small.beam_search_ex(W, N, p)) == "beam search: the state needs max_batch >= n_windows * beam_size decoder rows"
    assert message(lambda: small.sample_pass_n(W, 6, T_PASS, [1] * W, np.zeros((W, 6, ctx.hp.n_text_ctx)), p)) == "sample_pass_n: best_of must be in 1..5"
    assert message(lambda: small.beam_search(W, 6, p)) == "beam search: beam_size must be in 2..5"
    one = _state(E, ctx, 1)                           # the single-row loop has no row count of its own: its batch is the encode's
    _encode(E, one, pcm, 1)
    assert message(lambda: one.greedy_ex(W, p)) == "greedy: batch must equal the batch of the last ohw_encode"
    assert message(lambda: one.sample_pass(W, T_PASS, [1] * W, u1, p)) == "sample_pass: batch must equal the batch of the last ohw_encode"
