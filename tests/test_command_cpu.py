"""Command lists on the host (no GPU): the builder (ohw_command_table_build_host) against a Python trie, the library's rule
(ohw_command_rule_host) against the numpy restatement in command_ref.py word for word, ohw_command_match_host, the proof that
the comparison the GPU kernel test makes (every word of the buffer equal to the restatement) flags each injected fault on the
cases that test runs, and the argument checks that need no device.
"""
import math

import numpy as np
import pytest

import command_ref as R
from openhush_amd import engine as E


@pytest.fixture(scope="module", autouse=True)
def _lib():
    E.lib()


def _host_rule(table):
    def fn(phrases, penalty, history, n_cur, row, eot):
        return E.command_rule_host(table, penalty, history, n_cur, row, eot)
    return fn


@pytest.mark.parametrize("phrases", [R.LIST_A, R.LIST_B, R.LIST_C, [[7]], [list(range(16))], [[1, 2], [1, 2], [1]]],
                         ids=["A", "B", "C", "one token", "sixteen tokens", "duplicates"])
def test_builder_equals_a_python_trie(phrases):
    got, want = E.command_table_build_host(phrases, R.EOT).arrays(), R.trie(phrases)
    assert got["eot"] == R.EOT
    for k, v in want.items():
        assert np.array_equal(np.asarray(got[k]), np.asarray(v)), k
    # every prefix is a node, the root and the full phrases included; a terminal carries the lowest index that ends there
    assert got["depth_start"][1] == 1 and got["terminal"][0] == 0 and got["phrase_id"][0] == -1
    assert sorted(int(i) for i in got["phrase_id"] if i >= 0) == sorted({min(j for j, q in enumerate(phrases) if q == p) for p in phrases})


def test_builder_shapes_the_lists_are_there_for():
    a, b = E.command_table_build_host(R.LIST_A, R.EOT).arrays(), E.command_table_build_host(R.LIST_B, R.EOT).arrays()
    assert a["child_off"][1] > 256                                      # the root's children
    assert a["depth_start"][2] - a["depth_start"][1] > 64               # a depth that needs two rounds of the 64-way search
    assert b["depth_start"][3] - b["depth_start"][2] == 1024
    assert a["depth_start"][17] - a["depth_start"][16] == 1             # the 16-token phrase is a node of depth 16
    assert E.command_table_build_host([], R.EOT).arrays()["depth_start"].tolist() == [0] * 18


def test_builder_refusals_name_the_phrase():
    for phrases, what in (([[1], []], "phrase 1 has 0 tokens"), ([[1] * 17], "phrase 0 has 17 tokens"), ([[1], [2], [R.EOT]], "phrase 2: token 900"),
                          ([[-1]], "phrase 0: token -1"), ([[1]] * 1025, "1025 phrases")):
        with pytest.raises(E.WhisperError) as ex:
            E.command_table_build_host(phrases, R.EOT)
        assert ex.value.code == E.OHW_E_INVALID_ARG and what in str(ex.value), what


def test_host_rule_equals_the_restatement_on_every_listed_case():
    n_rows = n_lp = 0
    for gi, (gname, phrases, p, cases) in enumerate(R.groups()):
        table = E.command_table_build_host(phrases, R.EOT)
        lg, hist, n_cur, done, names = R.make_rows(cases, 100 + gi)
        for r, name in enumerate(names):
            want, wlp = R.rule(phrases, p, hist[r], int(n_cur[r]), lg[r, :R.N_VOCAB])
            got, glp = E.command_rule_host(table, p, hist[r], int(n_cur[r]), lg[r, :R.N_VOCAB], R.EOT)
            assert R.same_words(got, want), (gname, name)
            assert (glp is None) == (wlp is None), (gname, name)
            if wlp is not None:                                         # the host twin sums in double: float32's rounding of the result is all that separates them
                assert glp == wlp or abs(glp - wlp) <= 2.0 ** -23 * max(1.0, abs(wlp)), (gname, name)
                n_lp += 1
            n_rows += 1
    assert n_rows >= 50 and n_lp >= 10


def test_host_rule_equals_the_restatement_on_random_rows():
    rng = np.random.default_rng(7)
    phrases = [[int(t) for t in rng.integers(0, 12, rng.integers(1, 5))] for _ in range(40)]      # a small alphabet: histories hit nodes
    table = E.command_table_build_host(phrases, R.EOT)
    on = 0
    for i in range(200):
        n = int(rng.integers(0, 7))
        hist = np.where(rng.random(16) < 0.25, R.TS, rng.integers(0, 12, 16)).astype(np.int32)
        row = (rng.standard_normal(R.N_VOCAB) * 3).astype(np.float32)
        p = [0.5, 100.0, math.inf][i % 3]
        want, wlp = R.rule(phrases, p, hist, n, row)
        got, glp = E.command_rule_host(table, p, hist, n, row, R.EOT)
        assert R.same_words(got, want), i
        assert (glp is None) == (wlp is None) and (wlp is None or abs(glp - wlp) <= 2.0 ** -23 * max(1.0, abs(wlp)))
        on += int(want[R.EOT] == row[R.EOT] and not R.same_words(want[:12], row[:12] - np.float32(p)))
    assert on > 20                                                      # rows on the list with a child took part


def test_what_the_cases_are_there_for():
    """stated on the restatement itself: which columns each case leaves alone"""
    cases = R.cases_a()
    zero = np.zeros(R.N_VOCAB, np.float32)

    def kept(name, p=7.5, phrases=R.LIST_A, cs=cases):
        out, lp = R.rule(phrases, p, cs[name][0], cs[name][1], zero)
        return sorted(int(i) for i in np.flatnonzero(out[:R.EOT + 1] == 0)), lp
    root = [10, 20, 30, 60] + list(range(100, 400))
    assert kept("empty") == (root, pytest.approx(math.log(len(root) / R.EOT)))
    assert kept("timestamp only")[0] == root and kept("timestamp only")[1] is not None
    assert kept("mid phrase behind a timestamp") == ([21], None) and kept("mid phrase, poison behind n_cur") == ([21], None)
    assert kept("prefix of another, timestamps between") == ([22, R.EOT], None)
    assert kept("whole phrase")[0] == [R.EOT] and kept("one token phrase")[0] == [R.EOT]
    assert kept("depth 15")[0] == [45] and kept("depth 16")[0] == [R.EOT]
    assert kept("17 text tokens")[0] == kept("17 text tokens of a listed start")[0] == kept("off the list")[0] == [R.EOT]
    assert kept("listed tail behind an unlisted token")[0] == [R.EOT]
    assert kept("first of 304")[0] == kept("inside 304")[0] == kept("last of 304")[0] == kept("behind the 304")[0] == [R.EOT]
    assert kept("n_cur = max_tokens")[0] == [22, R.EOT]
    out, _ = R.rule(R.LIST_A, math.inf, cases["mid phrase behind a timestamp"][0], 2, zero)
    assert out[21] == 0 and out[20] == R.BAN and out[R.EOT] == R.BAN and out[R.EOT + 1] == 0 and out[R.TS] == 0
    b = R.cases_b()
    assert kept("first of 1024", 100.0, R.LIST_B, b)[0] == kept("inside 1024", 100.0, R.LIST_B, b)[0] == [R.EOT]
    assert kept("depth 1 of 32", 100.0, R.LIST_B, b)[0] == list(range(600, 632))
    assert kept("not among 1024", 100.0, R.LIST_B, b)[0] == kept("three tokens", 100.0, R.LIST_B, b)[0] == [R.EOT]
    # -inf means "never": it enters neither sum, and children that are all -inf give -inf
    c = R.cases_c()
    lg, hist, n_cur, done, names = R.make_rows(c, 3)
    lps = {name: R.rule(R.LIST_C, 1000.0, hist[r], int(n_cur[r]), lg[r, :R.N_VOCAB])[1] for r, name in enumerate(names)}
    assert lps["all children -inf"] == -math.inf and lps["every text column -inf"] == -math.inf and lps["mid"] is None
    assert math.isfinite(lps["one child -inf"]) and lps["one child -inf"] < 0


@pytest.mark.parametrize("fault", R.FAULTS)
def test_the_buffer_comparison_flags_each_injected_fault(fault):
    """the GPU test asserts same_words(kernel's buffer, expected()): a kernel with this fault leaves expected(fault=...), which
    must differ from expected() in some group"""
    flagged = []
    for gi, (gname, phrases, p, cases) in enumerate(R.groups()):
        lg, hist, n_cur, done, names = R.make_rows(cases, 10 * gi)
        good, _ = R.expected(phrases, p, lg, hist, n_cur, done)
        bad, _ = R.expected(phrases, p, lg, hist, n_cur, done, fault=fault)
        flagged += [(gname, names[r]) for r in range(len(names)) if not R.same_words(good[r], bad[r])]
        assert R.same_words(good[len(names)], lg[len(names)])            # the guard row is nobody's
    assert flagged, fault
    if fault == "penalty_twice":                                         # a hard list has nothing to apply twice
        assert all("inf" not in g for g, _ in flagged)


def test_match_host():
    t = E.command_table_build_host(R.LIST_A, R.EOT)
    assert E.command_match_host(t, [20, 21]) == 1                       # the lowest index among duplicates (1 and 4)
    assert E.command_match_host(t, [R.TS, 20, 21, 22, R.TS2, R.EOT]) == 2
    assert E.command_match_host(t, [10]) == 0 and E.command_match_host(t, R.LONG) == 3 and E.command_match_host(t, [399]) == 305
    assert E.command_match_host(t, [20]) == -1 and E.command_match_host(t, []) == -1 and E.command_match_host(t, [R.TS, R.EOT]) == -1
    assert E.command_match_host(t, [11, 20, 21]) == -1 and E.command_match_host(t, R.LONG + [30]) == -1 and E.command_match_host(t, [20, 21, 21]) == -1


def test_host_rule_refusals():
    t = E.command_table_build_host(R.LIST_C, R.EOT)
    row = np.zeros(R.N_VOCAB, np.float32)
    for p in (0.0, -1.0, float("nan"), 1000.5, -math.inf):
        with pytest.raises(E.WhisperError) as ex:
            E.command_rule_host(t, p, [], 0, row, R.EOT)
        assert ex.value.code == E.OHW_E_INVALID_ARG, p
    for p in (1e-3, 1000.0, math.inf):
        E.command_rule_host(t, p, [], 0, row, R.EOT)
    with pytest.raises(E.WhisperError):
        E.command_rule_host(t, 1.0, [], -1, row, R.EOT)
    t.child_tok[0] = 30                                                  # children out of order: not a table the builder made
    with pytest.raises(E.WhisperError):
        E.command_rule_host(t, 1.0, [], 0, row, R.EOT)
    for good, bad in (("100", None), ("inf", None), ("0.5", None), (None, "0"), (None, "-3"), (None, "nan"), (None, "1001"), (None, "x")):
        if good:
            assert E.command_penalty_arg(good) == float(good)
        else:
            with pytest.raises(ValueError):
                E.command_penalty_arg(bad)
    assert E.parse_commands("lights on\n\n# a comment\n  lights off  \r\n") == ["lights on", "lights off"]
