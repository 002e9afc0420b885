"""Repetition penalty and no-repeat n-grams on the host (no GPU): the library's rule (ohw_repeat_rule_host) against the numpy
restatement in repeat_ref.py word for word, the restatement against transformers' two logits processors, the proof that the
comparison the GPU kernel test makes (every word of the buffer equal to the restatement) flags each injected fault on the cases
that test runs, and the argument checks that need no device.
"""
import numpy as np
import pytest

import repeat_ref as R
from openhush_amd import engine as E


@pytest.fixture(scope="module", autouse=True)
def _lib():
    E.lib()


def test_host_rule_equals_the_restatement_on_every_listed_case():
    n_rows = 0
    for gi, (gname, theta, n, cases) in enumerate(R.groups()):
        lg, hist, n_cur, done, names = R.make_rows(cases, 100 + gi)
        for r, name in enumerate(names):
            want = R.rule(theta, n, hist[r], int(n_cur[r]), lg[r, :R.N_VOCAB])
            got = E.repeat_rule_host(theta, n, hist[r], int(n_cur[r]), lg[r, :R.N_VOCAB], R.EOT)
            assert R.same_words(got, want), (gname, name)
            n_rows += 1
    assert n_rows >= 40


def test_what_the_cases_are_there_for():
    """stated on the restatement itself"""
    g = {name: (theta, n, cases) for name, theta, n, cases in R.groups()}
    zero = np.zeros(R.N_VOCAB, np.float32)

    def banned(group, case):
        theta, n, cases = g[group]
        out = R.rule(theta, n, cases[case][0], cases[case][1], zero)
        return sorted(int(i) for i in np.flatnonzero(out == R.BAN))
    assert banned("ban3", "empty_history") == banned("ban3", "n_cur_is_n_minus_2") == banned("ban3", "n_cur_is_n_minus_1") == []
    assert banned("ban3", "n_cur_is_n_no_match") == [] and banned("ban3", "aaa") == [5] and banned("ban3", "poison_completes_tail") == []
    assert banned("ban3", "only_start_is_0") == [22] and banned("ban3", "only_start_is_last") == [30]
    assert banned("ban3", "timestamp_in_tail") == [8] and banned("ban3", "timestamp_follower") == [] and banned("ban3", "two_followers") == [50, 51]
    assert banned("ban3", "n_cur_at_max_tokens") == [62]
    assert banned("ban1", "n1_bans_every_text_token") == [5, 6, 899] and banned("ban1", "n1_empty") == []
    assert banned("ban2", "aa_n2") == [5] and banned("ban2", "aaa_n2") == [5] and banned("ban2", "n2_no_tail_needed_yet") == []
    assert banned("ban32", "stretch_repeats") == [R.STRETCH[35]] and banned("ban32", "stretch_exactly_n") == [70]
    assert banned("ban32", "stretch_one_short") == banned("ban32", "stretch_breaks") == []
    # the penalty: once per distinct token, the sign decides, zeros keep their sign, timestamps stay
    row = zero.copy()
    row[[5, 6, R.TS]] = [3.25, -1.75, 4.0]
    out = R.rule(1.3, 0, [5, 6, 5, 5, R.TS, 5], 6, row)
    assert out[5] == np.float32(np.float32(3.25) / np.float32(1.3)) and out[6] == np.float32(np.float32(-1.75) * np.float32(1.3)) and out[R.TS] == 4.0
    z = R.rule(0.5, 0, [7, 8], 2, np.asarray([0.0] * 7 + [0.0, -0.0], np.float32))
    assert not np.signbit(z[7]) and np.signbit(z[8])
    # penalised and banned: the ban wins; with theta = 1.0 nothing but the ban moves
    theta, n, cases = g["pen1.3_ban2"]
    row = zero.copy()
    row[[5, 6]] = [-1.0, 2.0]
    out = R.rule(theta, n, cases["penalised_and_banned"][0], 3, row)
    assert out[6] == R.BAN and out[5] == np.float32(np.float32(-1.0) * np.float32(1.3))
    rng = np.random.default_rng(0)
    row = rng.standard_normal(R.N_VOCAB).astype(np.float32)
    out = R.rule(1.0, 3, [5, 5, 5], 3, row)
    assert out[5] == R.BAN and R.same_words(np.delete(out, 5), np.delete(row, 5))


@pytest.mark.parametrize("n", [1, 2, 3, 5])
@pytest.mark.parametrize("theta", [0.5, 1.0, 1.3, 2.0])
def test_restatement_equals_the_two_processors_of_transformers(theta, n):
    """random text-only histories over a small alphabet (so that n-grams repeat) and fp32 rows; -inf maps to OHW_REPEAT_BAN; the
    run-of-one-token history a a a, where start and tail overlap, is among them"""
    torch = pytest.importorskip("torch")
    tr = pytest.importorskip("transformers")
    pen = tr.RepetitionPenaltyLogitsProcessor(penalty=float(theta))
    ban = tr.NoRepeatNGramLogitsProcessor(n)
    rng = np.random.default_rng(1000 * n + int(10 * theta))
    V = 61
    histories = [[3, 3, 3], [3] * 9, [3, 4] * 6, []] + [[int(t) for t in rng.integers(0, 6, int(rng.integers(1, 40)))] for _ in range(40)]
    n_banned = 0
    for h in histories:
        row = (rng.standard_normal(V) * 3).astype(np.float32)
        row[rng.integers(0, 6)] = 0.0
        want = R.rule(theta, n, np.asarray(h + [0], np.int32), len(h), row, eot=V)
        if h:
            ids = torch.tensor([h], dtype=torch.long)
            sc = torch.from_numpy(row.copy())[None, :]
            sc = ban(ids, pen(ids, sc))
            got = sc[0].numpy().copy()
        else:
            got = row.copy()                     # the processors take no empty sequence; the rule leaves the row alone
        n_banned += int(np.isneginf(got).sum())
        got[np.isneginf(got)] = R.BAN
        assert R.same_words(got, want), h
        assert R.same_words(E.repeat_rule_host(theta, n, h, len(h), row, V), want), h
    assert n_banned > 0


@pytest.mark.parametrize("fault", R.FAULTS)
def test_the_kernel_tests_comparison_flags_every_injected_fault(fault):
    """A kernel with one of these faults produces, on the GPU test's own buffers, words that differ from the restatement: the
    faulty rule is run in numpy in the kernel's place and THE comparison of test_gpu_repeat_rule.py (same_words over the whole
    buffer) must fail, on the case built for the fault at least."""
    flagged = []
    for gi, (gname, theta, n, cases) in enumerate(R.groups()):
        for k, chunk in enumerate(R.chunks(cases)):
            lg, hist, n_cur, done, names = R.make_rows(chunk, 10 * gi + k)
            want = R.expected(theta, n, lg, hist, n_cur, done)
            bad = R.expected(theta, n, lg, hist, n_cur, done, fault)
            assert R.same_words(bad[-1], want[-1])                     # the guard row is done
            flagged += [f"{gname}/{names[r]}" for r in range(len(names)) if not R.same_words(bad[r], want[r])]
    must = {"per_occurrence": ["pen1.3/seven_times_once", "pen0.5/long_history"],
            "skips_last_start": ["ban3/aaa", "ban3/only_start_is_last", "ban2/aa_n2", "ban32/stretch_exactly_n"],
            "reads_n_cur": ["ban3/poison_completes_tail", "ban2/aaa_n2"],
            "bans_timestamp": ["ban3/timestamp_follower", "ban1/n1_bans_every_text_token"],
            "penalises_timestamp": ["pen1.3/timestamps_not_penalised", "pen0.5/timestamps_not_penalised"],
            "ban_before_penalty": ["pen1.3_ban2/penalised_and_banned", "pen0.5_ban3/penalised_and_banned_n3"]}[fault]
    assert set(must) <= set(flagged), (fault, flagged)


def test_mapping_expectation_uses_the_mapped_history():
    """expected() under the beam mappings reads history row r * row_mul and entry r * row_mul // group"""
    rng = np.random.default_rng(4)
    K = 5
    lg = rng.standard_normal((3, R.LD)).astype(np.float32)
    hist = np.zeros((3 * K, R.MAX_TOKENS), np.int32)
    hist[0, :3], hist[K, :3], hist[1, :3] = [5, 5, 5], [6, 6, 6], [7, 7, 7]
    out = R.expected(1.0, 3, lg, hist, np.asarray([3, 3, 0]), np.asarray([0, 0, 1]), None, K, K)
    assert out[0, 5] == R.BAN and out[1, 6] == R.BAN and out[1, 7] != R.BAN and R.same_words(out[2], lg[2])
    assert R.same_words(R.expected(1.0, 3, lg, hist, None, np.asarray([0, 0, 1]), None, K, K), lg)


def test_argument_checks_that_need_no_device():
    L = E.lib()
    bad = [(0.0099, 0), (100.5, 0), (float("nan"), 0), (float("inf"), 3), (-1.3, 0), (0.0, 0), (1.0, -1), (1.3, 33)]
    for theta, n in bad:
        for fn in (L.ohw_state_set_repeat_rule, L.ohw_engine_set_repetition):
            assert fn(None, theta, n) == E.OHW_E_INVALID_ARG
            assert b"repeat rule" in L.ohw_last_error(), (theta, n, L.ohw_last_error())       # the values are refused ahead of the handle
        with pytest.raises(E.WhisperError) as ex:
            E.repeat_rule_host(theta, n, [1, 2], 2, np.zeros(8, np.float32), 4)
        assert ex.value.code == E.OHW_E_INVALID_ARG
    for theta, n in [(0.01, 0), (100.0, 32), (1.0, 0)]:                  # the limits are inside; a null handle is still refused
        assert L.ohw_state_set_repeat_rule(None, theta, n) == E.OHW_E_INVALID_ARG
        assert b"state is null" in L.ohw_last_error()
        assert L.ohw_engine_set_repetition(None, theta, n) == E.OHW_E_INVALID_ARG
        assert L.ohw_pool_set_repetition(None, theta, n) == E.OHW_E_INVALID_ARG
        E.repeat_rule_host(theta, n, [1, 2], 2, np.zeros(8, np.float32), 4)
    assert L.ohw_state_repeat_rule(None, None, None) == E.OHW_E_INVALID_ARG
    with pytest.raises(E.WhisperError):
        E.repeat_rule_host(1.3, 2, [1, 2], -1, np.zeros(8, np.float32), 4)
    # history ids outside the row are compared, never written
    out = E.repeat_rule_host(1.3, 1, [99, -4, 2], 3, np.ones(8, np.float32), 4)
    assert out[2] == R.BAN and np.count_nonzero(out != 1.0) == 1
