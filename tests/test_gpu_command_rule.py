"""command_rule_kernel alone, through ohw_dbg_command_rule: the words it leaves in sentinel-guarded rows must equal the numpy
restatement (command_ref.py) exactly - one float32 subtraction each - under all three row mappings, and list_logprob must lie
within the tolerance command_ref.py derives from the kernel's reduction shape, written by a window's first row at steps without a
text token and by nobody else.

Size: n_vocab 1003 in rows of ld 1024 (guard columns [1003, 1024)), at most 21 case rows and a guard row per launch, max_tokens
448; one launch at 51866 columns in rows of 51872.  The beam mappings run K = 3 rows for each of four entries.
tests/test_command_cpu.py shows that this file's comparison flags each of nine injected faults on these same buffers.
"""
import math

import numpy as np
import pytest

import command_ref as R
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
def state(E):
    ctx = E.Context.synthetic(synth.PRESETS["nano"].as_list(), 1234, 0, E.OHW_DTYPE_F16)
    return E.State(ctx, 1)


def _wrong_rows(got, want, names):
    return [(names + ["guard row"])[r] for r in range(got.shape[0]) if not R.same_words(got[r], want[r])]


@pytest.mark.parametrize("gi", range(len(R.groups())), ids=[g[0] for g in R.groups()])
def test_listed_cases_equal_the_restatement(E, state, gi):
    """per (list, penalty): the root (more than 256 children), histories of timestamps only, mid phrase, a phrase that is a prefix
    of another with timestamps between its tokens, phrases of 1 and 16 tokens, 17 text tokens, off the list, a listed tail behind an
    unlisted token, a depth of 304 and one of 1024 nodes at their ends and past them, n_cur = max_tokens, poison behind n_cur, a done
    row, -inf columns, finite penalties and +inf; guard columns and the guard row untouched"""
    gname, phrases, p, cases = R.groups()[gi]
    table = E.command_table_build_host(phrases, R.EOT)
    lg, hist, n_cur, done, names = R.make_rows(cases, 10 * gi)
    assert lg.shape == (len(names) + 1, R.LD) and hist.shape[1] == R.MAX_TOKENS
    got, lp = state.dbg_command_rule(lg, R.N_VOCAB, hist, n_cur, done, table, p, R.EOT, sentinel=float(R.SENTINEL))
    want, wlp = R.expected(phrases, p, lg, hist, n_cur, done)
    print(gname, "list_logprob", lp.tolist(), "float64", wlp.tolist(), "tolerance", R.lp_tol(R.EOT))
    assert _wrong_rows(got, want, names) == [], gname
    assert not R.same_words(want, lg)                                    # the launch did something
    assert R.lp_agree(lp, wlp, R.EOT), (gname, lp, wlp)
    no_text = [not done[r] and not any(0 <= t < R.EOT for t in hist[r, :n_cur[r]]) for r in range(len(names))]
    assert any(no_text) and [w != float(R.SENTINEL) for w in wlp[:len(names)]] == no_text and lp[len(names)] == R.SENTINEL


def test_51866_columns(E, state):
    """large-v3's row: 50 columns per thread in the two sums, 1621 words of children bits"""
    n_vocab, ld, eot = 51866, 51872, 50257
    phrases = [[31, 32], [50000, 7], [50256], [12345, 12346, 12347]] + [[t] for t in range(20000, 20300)]
    table = E.command_table_build_host(phrases, eot)
    ts = eot + 108
    hists = {"empty": [], "timestamp": [ts], "mid": [ts, 12345], "last text id": [50256], "off": [50255]}
    rng = np.random.default_rng(5)
    rows = len(hists)
    lg = np.full((rows + 1, ld), R.SENTINEL, np.float32)
    lg[:rows, :n_vocab] = (rng.standard_normal((rows, n_vocab)) * 3).astype(np.float32)
    lg[1, [31, 40000, 50256]] = -np.inf
    hist = np.zeros((rows + 1, R.MAX_TOKENS), np.int32)
    n_cur = np.zeros(rows + 1, np.int32)
    for r, h in enumerate(hists.values()):
        hist[r, :len(h)], n_cur[r] = h, len(h)
    done = np.asarray([0] * rows + [1], np.int32)
    got, lp = state.dbg_command_rule(lg, n_vocab, hist, n_cur, done, table, 100.0, eot, sentinel=float(R.SENTINEL))
    want, wlp = R.expected(phrases, 100.0, lg, hist, n_cur, done, n_vocab, eot)
    print("list_logprob", lp.tolist(), "float64", wlp.tolist(), "tolerance", R.lp_tol(eot))
    assert _wrong_rows(got, want, list(hists)) == []
    assert R.lp_agree(lp, wlp, eot), (lp, wlp)
    assert [w != float(R.SENTINEL) for w in wlp] == [True, True, False, False, False, False]


def _beam_buffers(K):
    """four entries of K = 3 beams, the last one done: the beams of an entry share n_cur and nothing else"""
    T = R.TS
    per_entry = [[[], [], []],
                 [[T, 20], [T, R.TS2], [20, 21]],                        # beam 1 holds no text token and is not the window's first row
                 [[T, T, R.TS2], [20, T, 21], [20, 21, 22]],             # beam 0 holds no text token
                 [[20], [20], [20]]]
    hist = np.full((4 * K, R.MAX_TOKENS), 21, np.int32)                  # poison: 21 behind every history
    n_cur = np.zeros(4, np.int32)
    for w, beams in enumerate(per_entry):
        n_cur[w] = len(beams[0])
        for b, h in enumerate(beams[:K]):
            hist[w * K + b, :len(h)] = h
    return hist, n_cur, np.asarray([0, 0, 0, 1], np.int32)


@pytest.mark.parametrize("p", [7.5, math.inf])
def test_beam_step_mapping_rows_of_a_window_share_its_length(E, state, p):
    """row_mul = 1, group = K: launch row r = decoder row r, entry r // K; the entry's first row alone writes list_logprob"""
    K = 3
    hist, n_cur, done = _beam_buffers(K)
    table = E.command_table_build_host(R.LIST_A, R.EOT)
    rng = np.random.default_rng(6)
    lg = np.full((4 * K, R.LD), R.SENTINEL, np.float32)
    lg[:3 * K, :R.N_VOCAB] = (rng.standard_normal((3 * K, R.N_VOCAB)) * 3).astype(np.float32)
    got, lp = state.dbg_command_rule(lg, R.N_VOCAB, hist, n_cur, done, table, p, R.EOT, row_mul=1, group=K, sentinel=float(R.SENTINEL))
    want, wlp = R.expected(R.LIST_A, p, lg, hist, n_cur, done, row_mul=1, group=K)
    assert _wrong_rows(got, want, [f"w{r // K}b{r % K}" for r in range(4 * K)][:-1]) == []
    assert [not R.same_words(want[r], lg[r]) for r in range(4 * K)] == [True] * (3 * K) + [False] * K
    assert R.lp_agree(lp, wlp, R.EOT), (lp, wlp)
    assert [w != float(R.SENTINEL) for w in wlp] == [True, False, True, False]


def test_first_beam_step_mapping_one_row_per_window(E, state):
    """row_mul = K, group = K: launch row r changes logits row r with the history of decoder row r * K, entry r"""
    K = 3
    hist, n_cur, done = _beam_buffers(K)
    table = E.command_table_build_host(R.LIST_A, R.EOT)
    rng = np.random.default_rng(9)
    lg = np.full((4, R.LD), R.SENTINEL, np.float32)
    lg[:3, :R.N_VOCAB] = (rng.standard_normal((3, R.N_VOCAB)) * 3).astype(np.float32)
    got, lp = state.dbg_command_rule(lg, R.N_VOCAB, hist, n_cur, done, table, 100.0, R.EOT, row_mul=K, group=K, sentinel=float(R.SENTINEL))
    want, wlp = R.expected(R.LIST_A, 100.0, lg, hist, n_cur, done, row_mul=K, group=K)
    assert _wrong_rows(got, want, ["w0", "w1", "w2"]) == []
    assert R.lp_agree(lp, wlp, R.EOT), (lp, wlp)
    assert [w != float(R.SENTINEL) for w in wlp] == [True, False, True, False]


def test_null_n_cur_means_every_history_is_empty_and_the_root_applies(E, state):
    hist, _, _ = _beam_buffers(1)
    table = E.command_table_build_host(R.LIST_C, R.EOT)
    lg = np.random.default_rng(2).standard_normal((4, R.LD)).astype(np.float32)
    got, lp = state.dbg_command_rule(lg, R.N_VOCAB, hist, None, [0, 0, 0, 1], table, math.inf, R.EOT, sentinel=float(R.SENTINEL))
    want, wlp = R.expected(R.LIST_C, math.inf, lg, hist, None, [0, 0, 0, 1])
    assert R.same_words(got, want) and R.lp_agree(lp, wlp, R.EOT)
    free = np.flatnonzero(got[0, :R.EOT + 1] != R.BAN).tolist()
    assert free == [10, 20] and wlp[3] == float(R.SENTINEL)


def test_bad_arguments_are_refused_before_the_launch(E, state):
    lg = np.zeros((2, 16), np.float32)
    hist = np.zeros((2, 8), np.int32)
    table = E.command_table_build_host([[1, 2], [3]], 10)
    ok = dict(n_vocab=16, histories=hist, n_cur=[0, 8], done=[0, 0], table=table, penalty=5.0, eot=10)
    state.dbg_command_rule(lg, **ok)
    for change in (dict(n_vocab=17), dict(n_cur=[0, 9]), dict(n_cur=[-1, 0]), dict(penalty=0.0), dict(penalty=float("nan")), dict(penalty=1001.0),
                   dict(penalty=-math.inf), dict(eot=-1), dict(row_mul=3), dict(row_mul=0)):
        with pytest.raises(E.WhisperError) as ex:
            state.dbg_command_rule(lg, **{**ok, **change})
        assert ex.value.code == E.OHW_E_INVALID_ARG, change
    big = np.zeros((2, 4097), np.int32)
    with pytest.raises(E.WhisperError):
        state.dbg_command_rule(lg, **{**ok, "histories": big})
    broken = E.command_table_build_host([[1, 2], [3]], 10)
    broken.child_off[1] = 7                                              # past the edges
    with pytest.raises(E.WhisperError):
        state.dbg_command_rule(lg, **{**ok, "table": broken})
    # the state's own list is in effect again after the test entry ran with another
    eot = int(state.ctx.tok.eot)
    assert state.command_count() == 0
    state.set_command_table([[1, 2, 3], [4]], 50.0)
    state.dbg_command_rule(lg, **ok)
    assert state.command_count() == 2
    state.set_command_table(None)
    assert state.command_count() == 0 and eot > 4
