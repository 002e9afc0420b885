"""The group form of the device temperature sampler (sampler_group_kernel through ohw_dbg_sample_group: N candidates per
window, best-of sampling) and the slot table of ohw_sample_pass_n.

sampler_group_kernel and sampler_t_kernel are ONE body (sampler_t_row<GROUP>): a row's arithmetic is the same code, so tokens and
log-probability words must be EQUAL to ohw_dbg_sample_t's on the same rows - by construction, and checked here.  What the group
form adds is checked on its own: the first step's shared logits row, per-row done flags, the window flag set by the row that
finishes last, inactive windows.  Shapes: the `nano` vocabulary rows of tests/golden/sampler.npz."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from openhush_amd import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from openhush_amd import engine
    engine.lib()
    return engine


@pytest.fixture(scope="module")
def nano(E):
    hp = synth.PRESETS["nano"]
    ctx = E.Context.synthetic(hp.as_list(), 1234, 0, E.OHW_DTYPE_F16)
    g = np.load(os.path.join(GOLDEN, "sampler.npz"))
    rows = g["rows_f16"].astype(np.float32)
    hists = [[int(t) for t in g["hists"][g["hist_of_row"][r]] if t >= 0] for r in range(rows.shape[0])]
    return ctx, rows, hists


def _words(x):
    return np.asarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize("N", [1, 2, 3, 5])
def test_group_rows_equal_the_single_form_word_for_word(E, nano, N):
    """later steps (every row its own logits row and history): the goldens' rows, padded to a multiple of N with repeats, through
    both entries with the same draws, with and without a logit bias, at three temperatures"""
    ctx, rows, hists = nano
    R = (rows.shape[0] + N - 1) // N * N
    idx = [r % rows.shape[0] for r in range(R)]
    lg, hs = rows[idx], [hists[i] for i in idx]
    st = E.State(ctx, R)
    p = ctx.default_params()
    rng = np.random.default_rng(9)
    picks = set()
    for use_bias in (False, True):
        bias = None
        if use_bias:
            bias = (rng.standard_normal(rows.shape[1]) * 1.5).astype(np.float32)
            bias[ctx.tok.timestamp_begin:] += 4.0
        st.set_logit_bias(bias)
        for T in (0.2, 0.6, 1.0):
            u = E.HostRng(31 + int(10 * T)).uniforms(R)
            t1, l1, _ = st.dbg_sample_t(p, lg, hs, T, u)
            g = st.dbg_sample_group(p, lg, hs, N, False, T, u, [0] * R)
            assert np.array_equal(g["tokens"], t1), (N, use_bias, T)
            assert np.array_equal(_words(g["logprobs"]), _words(l1)), (N, use_bias, T)
            ended = g["tokens"] == ctx.tok.eot
            assert np.array_equal(g["n_cur"], np.array([len(h) for h in hs]) + (~ended).astype(np.int32))
            assert np.array_equal(g["done"].astype(bool), ended)       # far from every length limit: done = end-of-text
            assert np.array_equal(g["win_done"], ended.reshape(-1, N).all(axis=1).astype(np.int32))
            picks.update(int(t) for t in t1)
    st.set_logit_bias(None)
    assert len(picks) > 10


@pytest.mark.parametrize("N", [2, 3, 5])
def test_first_step_reads_the_windows_row_for_all_its_candidates(E, nano, N):
    """first step: W prompt logits rows, N different draws each = ohw_dbg_sample_t on N copies of every row; the no-speech
    probability of every row is its window's.  The windows include the no-speech rows with real mass of
    test_temperature_kernel_against_the_host_sampler"""
    ctx, rows, _ = nano
    ns_rows = []
    for k, d in enumerate((-1.0, 0.5, 2.0)):
        x = rows[k].copy()
        x[ctx.tok.nosp] = x.max() + d
        ns_rows.append(x)
    # and two flat rows (unit-variance noise): the goldens' rows are peaked, N draws there mostly land on one token
    flat = (np.random.default_rng(2).standard_normal((2, rows.shape[1]))).astype(np.float32)
    win = np.concatenate([rows[:4], np.stack(ns_rows), flat])
    W = win.shape[0]
    R = W * N
    st = E.State(ctx, R)
    p = ctx.default_params()
    for T in (0.4, 1.0):
        u = E.HostRng(5).uniforms(R)
        copies = np.repeat(win, N, axis=0)
        t1, l1, n1 = st.dbg_sample_t(p, copies, [[] for _ in range(R)], T, u)
        g = st.dbg_sample_group(p, win, [[] for _ in range(R)], N, True, T, u, [0] * R)
        assert np.array_equal(g["tokens"], t1) and np.array_equal(_words(g["logprobs"]), _words(l1)), T
        assert np.array_equal(_words(g["no_speech_prob"]), _words(n1)), T
        assert float(g["no_speech_prob"].max()) > 0.3                                          # the no-speech rows really carry mass
        assert all(len(set(int(t) for t in t1[w * N:(w + 1) * N])) == N for w in (W - 2, W - 1))      # the draws differ within a window
        for w in range(W):
            assert len(set(_words(g["no_speech_prob"][w * N:(w + 1) * N]).tolist())) == 1


def test_window_flag_is_set_by_the_row_that_finishes_last(E, nano):
    """three windows of N = 3 over four steps.  A row ends when its draw lands on end-of-text, which a bias makes nearly certain for
    the rows whose turn it is (their history allows it) - rows of one window end on different steps; the window's flag rises with
    its last row and not before; a row that is done neither writes nor advances; an inactive window starts done"""
    ctx, rows, hists = nano
    N, W = 3, 3
    R = N * W
    V = rows.shape[1]
    eot, tb = ctx.tok.eot, ctx.tok.timestamp_begin
    st = E.State(ctx, R)
    p = ctx.default_params()
    base = rows[0]
    end_row = base.copy(); end_row[eot] = base.max() + 60.0          # end-of-text with probability ~1
    go_row = base.copy(); go_row[eot] = base.min() - 60.0            # never end-of-text
    hist = [[tb, 100 + r] for r in range(R)]                         # an open segment: text, timestamps and end-of-text all allowed
    # step on which each row ends (0: never within the four steps); window 2 is inactive
    ends_at = [1, 3, 2,   2, 2, 4,   0, 0, 0]
    done = np.array([0] * 6 + [1] * 3, np.int32)
    g0 = st.dbg_sample_group(p, np.stack([go_row] * R), hist, N, False, 1.0, [0.5] * R, done)
    assert list(g0["win_done"]) == [0, 0, 1] and list(g0["done"]) == list(done)                # the inactive window starts done
    n_cur = np.array([len(h) for h in hist])
    for step in range(1, 5):
        lg = np.stack([end_row if ends_at[r] == step else go_row for r in range(R)])
        g = st.dbg_sample_group(p, lg, hist, N, False, 1.0, [0.5] * R, done)
        for r in range(R):
            if done[r]:
                # already done: no token, no log-probability, no history growth
                assert g["tokens"][r] == 0 and g["logprobs"][r] == 0.0 and g["n_cur"][r] == n_cur[r], (step, r)
            elif ends_at[r] == step:
                assert g["tokens"][r] == eot and g["done"][r] == 1 and g["n_cur"][r] == n_cur[r], (step, r)
            else:
                assert g["tokens"][r] != eot and g["done"][r] == 0 and g["n_cur"][r] == n_cur[r] + 1, (step, r)
                hist[r] = hist[r] + [int(g["tokens"][r])]
        n_cur = np.array([len(h) for h in hist])
        done = g["done"].copy()
        want = [int(all(0 < ends_at[w * N + j] <= step for j in range(N))) for w in range(2)] + [1]
        assert list(g["win_done"]) == want, (step, list(g["win_done"]), want)
    assert list(done) == [1, 1, 1, 1, 1, 1, 1, 1, 1] and want == [1, 1, 1]


def _slots_ref(W, N, C, shared, stride):
    tab = np.empty((W * N, C), np.int32)
    for r in range(W * N):
        w = r // N
        tab[r, :] = r
        tab[r, :shared[w]] = w * stride
    return tab


@pytest.mark.parametrize("N", [2, 3, 5])
def test_slot_table_for_unequal_shared_lengths(E, nano, N):
    """fetch("sample_slots") after ohw_sample_pass_n against a numpy restatement: context lengths 0, 5 and 11 in one batch (the
    windows' pasts move to rows w * N) and each alone (no move: the past stays in row 0), and with no context table at all"""
    ctx, _, _ = nano
    hp = synth.PRESETS["nano"]
    C = hp.n_text_ctx
    p = ctx.default_params(); p.n_max = 4
    n_prompt = 3 if hp.n_vocab >= 51865 else 1
    lens = [0, 5, 11]
    ctxs = [[100 + 7 * w + i for i in range(n)] for w, n in enumerate(lens)]

    def run(st, W, table):
        st.mel(np.stack([synth.synth_audio(60 + w) for w in range(W)]), None, E.OHW_MEL_REFLECT, want=False)
        st.encode(W)
        st.set_window_prompt(table)
        u = np.stack([E.HostRng(j).uniforms(C) for j in range(N)] * W).reshape(W, N, C)
        st.sample_pass_n(W, N, 0.6, [1] * W, u, p)
        return st.fetch("sample_slots", W * N)

    st3 = E.State(ctx, 3 * N)
    # [prev] leads a non-empty context: its shared length is len + 1 + n_prompt
    shared = [n_prompt + (n + 1 if n else 0) for n in lens]
    assert np.array_equal(run(st3, 3, ctxs), _slots_ref(3, N, C, shared, N))
    assert np.array_equal(run(st3, 3, None), _slots_ref(3, N, C, [n_prompt] * 3, 1))
    with pytest.raises(E.WhisperError):
        st3.fetch("sample_slots", 3 * N - 1)
    st1 = E.State(ctx, N)
    for w in range(3):
        assert np.array_equal(run(st1, 1, [ctxs[w]]), _slots_ref(1, N, C, [shared[w]], 1)), w
