"""Hot phrases on the host (no GPU): the library's builder (ohw_phrase_table_build_host) and rule (ohw_phrase_boost_host)
against the numpy restatement in phrase_ref.py, every refusal of the builder, the two tokenisations of the text form, the
hot-phrase file of the CLI, and the proof that the comparison the GPU kernel test makes (every word of the buffer equal to the
restatement) flags each injected fault on the cases that test runs.
"""
import numpy as np
import pytest

import phrase_ref as R
from openhush_amd import engine as E


@pytest.fixture(scope="module", autouse=True)
def _lib():
    E.lib()


def _random_table(rng, n_phrases, eot, alphabet):
    """phrases over a small alphabet, so that prefixes are shared, matches nest and edges collide"""
    phrases = [[int(t) for t in rng.choice(alphabet, size=int(rng.integers(1, R.MAX_LEN + 1)))] for _ in range(n_phrases)]
    boosts = [float(np.float32(rng.uniform(-3, 3))) for _ in range(n_phrases)]
    assert max(max(p) for p in phrases) < eot
    return phrases, boosts


@pytest.mark.parametrize("seed,n_phrases,n_alpha", [(0, 1, 3), (1, 7, 2), (2, 40, 3), (3, 200, 4), (4, 1024, 6)])
def test_builder_and_rule_equal_the_restatement_on_random_tables(seed, n_phrases, n_alpha):
    rng = np.random.default_rng(seed)
    alphabet = rng.choice(R.EOT, size=n_alpha, replace=False)
    phrases, boosts = _random_table(rng, n_phrases, R.EOT, alphabet)
    lib_t = E.phrase_table_build_host(phrases, boosts, R.EOT)
    ref_t = R.build(phrases, boosts)
    assert R.tables_equal(lib_t.arrays(), ref_t)
    matched_deeper = 0
    for _ in range(30):
        n_cur = int(rng.integers(0, R.MAX_TOKENS + 1))
        hist = rng.choice(np.concatenate([alphabet, [R.TS]]), size=R.MAX_TOKENS, p=[0.96 / n_alpha] * n_alpha + [0.04]).astype(np.int32)
        row = (rng.standard_normal(R.N_VOCAB) * 3).astype(np.float32)
        want = R.boost(ref_t, hist, n_cur, row)
        got = lib_t.boost_host(hist, n_cur, row)
        assert R.same_words(got, want)
        root_only = R.boost(ref_t, hist, 0, row)
        matched_deeper += int(not R.same_words(want, root_only))
    assert n_phrases < 7 or matched_deeper > 0


def test_listed_cases_on_the_host():
    for table, cases, nv, eot in ((R.base_table(), R.base_cases(), R.N_VOCAB, R.EOT), (R.wide_table(), R.wide_cases(), R.WIDE_VOCAB, R.WIDE_EOT)):
        lib_t = E.phrase_table_build_host(table[0], table[1], eot)
        ref_t = R.build(*table)
        assert R.tables_equal(lib_t.arrays(), ref_t)
        rng = np.random.default_rng(5)
        for name, (hist, n_cur, _) in cases.items():
            row = (rng.standard_normal(nv) * 3).astype(np.float32)
            assert R.same_words(lib_t.boost_host(hist, n_cur, row), R.boost(ref_t, hist, n_cur, row)), name
    # what the cases are there for, stated on the restatement itself
    t = R.build(*R.base_table())
    zero = np.zeros(R.N_VOCAB, np.float32)
    c = R.base_cases()
    changed = lambda name: {int(i): float(v) for i, v in enumerate(R.boost(t, c[name][0], c[name][1], zero)) if v != 0}
    root = {10: 1.5, 11: 2.25, 12: 4.0, 20: 3.0, 30: -1.25, 100: 0.5}
    assert changed("empty_history") == root and changed("empty_history_poison") == root
    assert changed("depth1") == {**root, 31: -1.25}
    assert changed("depth15") == {**root, 115: 0.5} == changed("depth15_exact_length")
    assert changed("shorter_than_depth") == {**root, 12: 4.0 + 2.25}
    assert changed("oldest_differs") == root
    assert changed("timestamp_in_tail") == {**root, 12: 4.0 + 2.25} and changed("timestamp_last") == root
    assert changed("nested") == {**root, 12: float(np.float32(np.float32(4.0 + 2.25) + np.float32(1.5))), 13: 0.75}      # root, [11], [10, 11]
    assert changed("poison_extends") == {**root, 11: 2.25 + 1.5}
    w = R.build(*R.wide_table())
    assert int(w["child_off"][2] - w["child_off"][1]) == 1024
    assert np.count_nonzero(R.boost(w, *R.wide_cases()["wide_node"][:2], np.zeros(R.WIDE_VOCAB, np.float32))) == 1025


def test_edge_boost_is_the_maximum_and_only_prefixes_with_a_continuation_are_nodes():
    t = E.phrase_table_build_host([[1, 2], [1, 2, 3], [1], [1, 2]], [0.5, -1.0, 0.25, 0.75], 10).arrays()
    assert list(t["depth_start"][:4]) == [0, 1, 2, 3] and t["depth_start"][16] == 3            # nodes: [], [1], [1, 2]; [1, 2, 3] is none
    assert list(t["child_tok"]) == [1, 2, 3] and [float(b) for b in t["child_boost"]] == [0.75, 0.75, -1.0]
    assert list(t["path"]) == [1, 1, 2]
    empty = E.phrase_table_build_host([], [], 10)
    assert empty.c.n_nodes == 0 and R.same_words(empty.boost_host([1, 2], 2, np.ones(10, np.float32)), np.ones(10, np.float32))


@pytest.mark.parametrize("phrases,boosts,needle", [
    ([[1], []], [1.0, 1.0], "phrase 1"),                               # a length of 0
    ([[1], [2], list(range(17))], [1.0, 1.0, 1.0], "phrase 2"),        # a length above 16
    ([[1, 100]], [1.0], "phrase 0"),                                   # an id at eot
    ([[1], [-1]], [1.0, 1.0], "phrase 1"),                             # a negative id
    ([[1], [2]], [1.0, float("inf")], "phrase 1"),                     # a boost that is not finite
    ([[1], [2]], [float("nan"), 1.0], "phrase 0"),
    ([[i % 50, i // 50] for i in range(1025)], [1.0] * 1025, "1025"),  # more than 1024 phrases
])
def test_builder_refusals_name_the_phrase(phrases, boosts, needle):
    with pytest.raises(E.WhisperError) as ex:
        E.phrase_table_build_host(phrases, boosts, 100)
    assert ex.value.code == E.OHW_E_INVALID_ARG and needle in str(ex.value), str(ex.value)
    E.phrase_table_build_host([list(range(16))], [1.0], 100)           # 16 tokens and 1024 phrases are inside the limits
    E.phrase_table_build_host([[i % 50, i // 50] for i in range(1024)], [1.0] * 1024, 100)


def test_rule_refuses_a_table_that_is_none():
    t = E.phrase_table_build_host([[1, 2]], [1.0], 10)
    with pytest.raises(E.WhisperError):
        t.boost_host([1], 1, np.zeros(2, np.float32))                  # child token 2 is outside a row of 2
    t.child_off[1] = 9
    with pytest.raises(E.WhisperError):
        t.boost_host([1], 1, np.zeros(10, np.float32))


class _Tok:
    """a stand-in for Context.tokenize: one token per byte, so the two variants differ by the space's token"""
    def tokenize(self, text):
        return [int(b) for b in E._text_bytes(text)]


def test_text_form_yields_the_two_variants_without_duplicates():
    phrases, boosts = E.hot_phrase_tokens(_Tok(), ["ab", " c", "ab"], [1.0, 2.0, 3.0])
    assert phrases == [[32, 97, 98], [97, 98], [32, 32, 99], [32, 99]]         # " ab", "ab", "  c", " c"; the second "ab" adds nothing
    assert boosts == [1.0, 1.0, 2.0, 2.0]
    assert E.hot_phrase_tokens(_Tok(), [[5, 6], [7]], 1.5) == ([[5, 6], [7]], [1.5, 1.5])
    class NoLetters(_Tok):                       # a vocabulary without letters: a form that has no token is dropped
        def tokenize(self, text):
            return [t for t in super().tokenize(text) if t == 32]
    assert E.hot_phrase_tokens(NoLetters(), ["ab", " "], 1.0) == ([[32], [32, 32]], [1.0, 1.0])
    class Nothing(_Tok):
        def tokenize(self, text):
            return []
    with pytest.raises(ValueError, match="text 0"):
        E.hot_phrase_tokens(Nothing(), ["ab", "cd"], 1.0)
    with pytest.raises(ValueError):
        E.hot_phrase_tokens(_Tok(), ["ab", [1]], 1.0)
    with pytest.raises(ValueError):
        E.hot_phrase_tokens(_Tok(), ["ab"], [1.0, 2.0])


def test_hot_phrase_file_with_and_without_boosts(tmp_path):
    text = "Kubernetes\nMI355X\t4.5\n\n# a comment\nopen hush \t 0.5\nplain\t\n"
    assert E.parse_hot_phrases(text, 2.0) == (["Kubernetes", "MI355X", "open hush", "plain"], [2.0, 4.5, 0.5, 2.0])
    with pytest.raises(ValueError, match="line 2"):
        E.parse_hot_phrases("a\nb\tmuch\n", 1.0)
    with pytest.raises(ValueError, match="line 1"):
        E.parse_hot_phrases("\t3\n", 1.0)
    # the flags of both commands reach the parser
    from openhush_amd import cli
    f = tmp_path / "phrases.txt"
    f.write_text(text, encoding="utf-8")
    import argparse
    for cmd in ("transcribe", "transcribe-many"):
        ap = argparse.ArgumentParser()
        cli._add_transcribe_options(ap)
        args = ap.parse_args(["--model-path", "m.bin", "--hot-phrases", str(f), "--hot-phrase-boost", "3"])
        assert cli._read_hot_phrases(args) == (["Kubernetes", "MI355X", "open hush", "plain"], [3.0, 4.5, 0.5, 3.0]), cmd
        assert cli._read_hot_phrases(ap.parse_args(["--model-path", "m.bin"])) == ()
    assert cli._read_hot_phrases(ap.parse_args(["--model-path", "m.bin", "--hot-phrases", str(tmp_path / "none.txt")])) is None


@pytest.mark.parametrize("fault", R.FAULTS)
def test_the_kernel_tests_comparison_flags_every_injected_fault(fault):
    """A kernel with one of these faults produces, on the GPU test's own buffers, words that differ from the restatement: the
    faulty rule is run in numpy in the kernel's place and THE comparison of test_gpu_phrase_boost.py (same_words over the whole
    buffer) must fail on at least one of its runs."""
    flagged = []
    for table, cases, nv, ld in ((R.base_table(), R.base_cases(), R.N_VOCAB, R.LD), (R.wide_table(), R.wide_cases(), R.WIDE_VOCAB, R.WIDE_LD)):
        t = R.build(*table)
        lg, hist, n_cur, done, names = R.make_rows(cases, 3, nv, ld)
        want = R.expected(t, lg, hist, n_cur, done, None, nv)
        bad = R.expected(t, lg, hist, n_cur, done, fault, nv)
        if not R.same_words(bad, want):
            flagged += [names[r] for r in range(len(names)) if not R.same_words(bad[r], want[r])]
    assert flagged, fault
    must = {"tail_off_by_one": "depth1", "reads_n_cur": "poison_extends", "drops_last_child": "wide_node", "deepest_only": "nested"}[fault]
    assert must in flagged, (fault, flagged)
    if fault == "reads_n_cur":
        assert "empty_history_poison" in flagged and "wide_poison" in flagged
