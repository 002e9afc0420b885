"""repeat_rule_kernel alone, through ohw_dbg_repeat_rule: the words it leaves in sentinel-guarded rows must equal the numpy
restatement (repeat_ref.py) exactly - float32 multiplies and divides, one rounding each - on every case the rule's definition
makes delicate.

Size: n_vocab 1003 in rows of ld 1024 (guard columns [1003, 1024)), at most 5 case rows and a guard row per launch, max_tokens
448; the two beam mappings need K = 5 rows for each of two windows and run 10 rows and a guard row.  tests/test_repeat_cpu.py
shows that this file's comparison flags a token penalised once per occurrence, the last start left out, a tail read at
tokens[n_cur], a banned timestamp follower, a penalised timestamp and the ban applied before the penalty on these same buffers.
"""
import numpy as np
import pytest

import repeat_ref as R
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
    """per (penalty, ngram) setting: empty history, n_cur = n - 2 / n - 1 / n, n = 1, n = 32 on a repeated 40-token stretch, 300-token
    histories whose only start is 0 or n_cur - n, a a a, a token seen 7 times, logits of either sign and both zeros, timestamps in
    the tail and as followers, a token penalised and banned, theta = 1.0 with n = 3, done rows, n_cur = max_tokens; guard columns and
    the guard row untouched"""
    gname, theta, n, cases = R.groups()[gi]
    moved = 0
    for k, chunk in enumerate(R.chunks(cases)):
        lg, hist, n_cur, done, names = R.make_rows(chunk, 10 * gi + k)
        assert lg.shape == (len(names) + 1, R.LD) and len(names) <= R.ROWS and hist.shape[1] == R.MAX_TOKENS
        got = state.dbg_repeat_rule(lg, R.N_VOCAB, hist, n_cur, done, theta, n, R.EOT)
        want = R.expected(theta, n, lg, hist, n_cur, done)
        assert _wrong_rows(got, want, names) == [], (gname, k)
        moved += int(not R.same_words(want, lg))
    assert moved > 0                                   # the launches did something


def test_theta_one_moves_no_word_but_the_banned(E, state):
    lg, hist, n_cur, done, names = R.make_rows({"aaa": R._case([5, 5, 5]), "seen": R._case([6, 7, 8, 9])}, 77)
    got = state.dbg_repeat_rule(lg, R.N_VOCAB, hist, n_cur, done, 1.0, 3, R.EOT)
    diff = np.argwhere(got.view(np.uint32) != lg.view(np.uint32))
    assert diff.tolist() == [[0, 5]] and got[0, 5] == R.BAN


def _beam_buffers(K, seed):
    """two windows of K beams with their own histories of the windows' lengths (7 and 12), window 1 done, and a guard entry"""
    rng = np.random.default_rng(seed)
    hist = rng.integers(0, 4, (3 * K, R.MAX_TOKENS)).astype(np.int32)       # a small alphabet: every beam repeats n-grams
    hist[:, ::5] = R.TS
    n_cur = np.asarray([7, 12, R.MAX_TOKENS], np.int32)
    return hist, n_cur


@pytest.mark.parametrize("done1", [0, 1])
def test_beam_step_mapping_rows_of_a_window_share_its_length(E, state, done1):
    """row_mul = 1, group = K: launch row r = decoder row r, entry r // K"""
    K = 5
    hist, n_cur = _beam_buffers(K, 5)
    done = np.asarray([0, done1, 1], np.int32)
    rng = np.random.default_rng(6)
    lg = np.full((2 * K + 1, R.LD), R.SENTINEL, np.float32)
    lg[:2 * K, :R.N_VOCAB] = (rng.standard_normal((2 * K, R.N_VOCAB)) * 3).astype(np.float32)
    got = state.dbg_repeat_rule(lg, R.N_VOCAB, hist, n_cur, done, 1.3, 2, R.EOT, row_mul=1, group=K)
    want = R.expected(1.3, 2, lg, hist, n_cur, done, None, 1, K)
    assert _wrong_rows(got, want, [f"w{r // K}b{r % K}" for r in range(2 * K)]) == []
    changed = [r for r in range(2 * K) if not R.same_words(want[r], lg[r])]
    assert changed == list(range(K if done1 else 2 * K))
    assert len({hist[r, :7].tobytes() for r in range(K)}) > 1                 # the beams of a window do not share a history


@pytest.mark.parametrize("done0", [0, 1])
def test_first_beam_step_mapping_one_row_per_window(E, state, done0):
    """row_mul = K, group = K: launch row r changes logits row r with the history of decoder row r * K, entry r"""
    K = 5
    hist, n_cur = _beam_buffers(K, 8)
    done = np.asarray([done0, 0, 1], np.int32)
    rng = np.random.default_rng(9)
    lg = np.full((3, R.LD), R.SENTINEL, np.float32)
    lg[:2, :R.N_VOCAB] = (rng.standard_normal((2, R.N_VOCAB)) * 3).astype(np.float32)
    got = state.dbg_repeat_rule(lg, R.N_VOCAB, hist, n_cur, done, 0.5, 3, R.EOT, row_mul=K, group=K)
    want = R.expected(0.5, 3, lg, hist, n_cur, done, None, K, K)
    assert _wrong_rows(got, want, ["w0", "w1"]) == []
    assert [not R.same_words(want[r], lg[r]) for r in range(3)] == [not done0, True, False]


def test_null_n_cur_means_every_history_is_empty(E, state):
    hist, _ = _beam_buffers(1, 3)
    lg = np.random.default_rng(2).standard_normal((3, R.LD)).astype(np.float32)
    got = state.dbg_repeat_rule(lg, R.N_VOCAB, hist, None, [0, 0, 0], 1.3, 1, R.EOT)
    assert R.same_words(got, lg)


def test_bad_arguments_are_refused_before_the_launch(E, state):
    lg = np.zeros((2, 16), np.float32)
    hist = np.zeros((2, 8), np.int32)
    ok = dict(n_vocab=16, histories=hist, n_cur=[0, 8], done=[0, 0], penalty=1.3, ngram=2, eot=10)
    state.dbg_repeat_rule(lg, **ok)
    for change in (dict(n_vocab=17), dict(n_cur=[0, 9]), dict(n_cur=[-1, 0]), dict(penalty=0.001), dict(penalty=float("nan")), dict(ngram=33),
                   dict(ngram=-1), dict(eot=-1), dict(row_mul=3), dict(row_mul=0)):
        with pytest.raises(E.WhisperError) as ex:
            state.dbg_repeat_rule(lg, **{**ok, **change})
        assert ex.value.code == E.OHW_E_INVALID_ARG, change
    big = np.zeros((2, 4097), np.int32)
    with pytest.raises(E.WhisperError):
        state.dbg_repeat_rule(lg, **{**ok, "histories": big})                # more history than the kernel's LDS holds
    # the state's own setting is in effect again after the test entry ran with other values
    state.set_repeat_rule(2.0, 4)
    state.dbg_repeat_rule(lg, **ok)
    assert state.repeat_rule() == (2.0, 4)
    state.set_repeat_rule()
    assert state.repeat_rule() == (1.0, 0)
