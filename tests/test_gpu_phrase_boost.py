"""phrase_boost_kernel alone, through ohw_dbg_phrase_boost: the words it leaves in sentinel-guarded rows must equal the numpy
restatement (phrase_ref.py) exactly - float32 adds in table order - on every case the rule's definition makes delicate.

Size: n_vocab 1003 in rows of ld 1024 (guard columns [1003, 1024)), at most 5 case rows and a guard row per launch.  A node
with 1024 children cannot exist in a vocabulary of 1003, so that one table runs at n_vocab 1091 / ld 1120 (phrase_ref.WIDE_*),
the smallest odd size that holds its 1024 text tokens.  tests/test_phrase_cpu.py shows that this file's comparison flags a
tail window off by one, a read of tokens[n_cur], a dropped last child and deepest-only matching on these same buffers.
"""
import numpy as np
import pytest

import phrase_ref as R
from openhush_amd import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROWS = 5       # case rows per launch; the guard row makes 6


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


def _chunks(cases):
    names = list(cases)
    return [{n: cases[n] for n in names[i:i + ROWS]} for i in range(0, len(names), ROWS)]


def _run(E, state, table, cases, seed, n_vocab=R.N_VOCAB, ld=R.LD, eot=R.EOT):
    """every chunk of the cases through the kernel -> the names of the rows whose words differ from the restatement"""
    lib_t = E.phrase_table_build_host(table[0], table[1], eot)
    ref_t = R.build(*table)
    assert R.tables_equal(lib_t.arrays(), ref_t)
    wrong = []
    for k, chunk in enumerate(_chunks(cases)):
        lg, hist, n_cur, done, names = R.make_rows(chunk, seed + k, n_vocab, ld)
        assert lg.shape[0] <= 6
        got = state.dbg_phrase_boost(lg, n_vocab, hist, n_cur, done, lib_t)
        want = R.expected(ref_t, lg, hist, n_cur, done, None, n_vocab)
        if not R.same_words(got, want):
            wrong += [(names + ["guard row"])[r] for r in range(lg.shape[0]) if not R.same_words(got[r], want[r])]
        # the launch did something: some live row differs from what went in
        assert any(not R.same_words(want[r], lg[r]) for r in range(len(names)) if not done[r]) or all(done[:len(names)])
    return wrong


def test_listed_cases_equal_the_restatement(E, state):
    """empty history, depth 1 and depth 15, a history shorter than a node's depth, a tail that differs in its oldest token, a
    timestamp inside the tail, nested matches that raise one token twice, poison at and behind n_cur, a done row, n_cur at
    max_tokens; guard columns and the guard row untouched"""
    assert _run(E, state, R.base_table(), R.base_cases(), 3) == []


def test_node_with_1024_children(E, state):
    """the child loop strides past the workgroup; the last child counts"""
    assert _run(E, state, R.wide_table(), R.wide_cases(), 7, R.WIDE_VOCAB, R.WIDE_LD, R.WIDE_EOT) == []


def test_two_tables_in_turn_on_the_same_buffers(E, state):
    """the device table is one fixed set of buffers: a small table after a large one must not see the large one's nodes
    (test_gpu_hot_phrases.py checks that a state's own table is in effect again after this test entry ran)"""
    rng = np.random.default_rng(9)
    alphabet = [3, 4, 5, 6]
    big = [[int(t) for t in rng.choice(alphabet, size=int(rng.integers(1, 17)))] for _ in range(600)]
    big_b = [float(np.float32(rng.uniform(0.5, 3))) for _ in big]
    small = ([[3, 4], [5]], [1.0, 2.0])
    cases = {f"h{i}": (np.asarray(rng.choice(alphabet, size=R.MAX_TOKENS), np.int32), int(rng.integers(0, R.MAX_TOKENS + 1)), 0) for i in range(5)}
    for table in ((big, big_b), small, (big, big_b), small):
        assert _run(E, state, table, cases, 21) == []


def test_bad_arguments_are_refused_before_the_launch(E, state):
    lib_t = E.phrase_table_build_host([[1, 2]], [1.0], 10)
    lg = np.zeros((1, 16), np.float32)
    hist = np.zeros((1, 8), np.int32)
    with pytest.raises(E.WhisperError):
        state.dbg_phrase_boost(lg, 2, hist, [0], [0], lib_t)            # child token 2 is outside n_vocab 2
    with pytest.raises(E.WhisperError):
        state.dbg_phrase_boost(lg, 17, hist, [0], [0], lib_t)           # n_vocab above ld
    with pytest.raises(E.WhisperError):
        state.dbg_phrase_boost(lg, 16, hist, [9], [0], lib_t)           # n_cur above max_tokens
    state.dbg_phrase_boost(lg, 16, hist, [8], [0], lib_t)
