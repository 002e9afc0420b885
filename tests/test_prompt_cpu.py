"""Prompted decoding, the parts that need no GPU: the tokenizer (ohw_tokenize_host) against a Python restatement of its rule
(tests/prompt_ref.py), the clipping rule, and the prefill's chunk plan against a cache model."""
import numpy as np
import pytest

import prompt_ref as R
from openhush_amd import engine as E
from openhush_amd import modelfile, synth

# 12 entries: overlapping prefixes (the longest wins), a leading-space form, a contraction, digits, one multi-byte letter
HAND = [b"a", b"ab", b"abc", b" ab", b"'", b"'ll", b"1", b"12", b" ", b"b", b"\xc3\xa9", b"c"]
TEXTS = [
    b"abcab",                 # overlapping entries: abc, then ab
    b" abab",                 # the leading space joins the word: " ab", "ab"
    b"ab'll a",               # contraction piece "'ll"; then " " and "a" (no " a" entry)
    b"a'x",                   # an apostrophe that starts no contraction: "'" alone, x has no entry
    b"121 2",                 # digits: 12, 1, then " " + (2: no entry -> skipped)
    b"abz\x01c",              # bytes with no entry are skipped
    b"\xc3\xa9ab",            # bytes >= 0x80 are letters: one piece, two tokens
    b"a  b",                  # a run of spaces is one piece
    b"",
]


@pytest.mark.parametrize("text", TEXTS)
def test_tokenize_hand_vocabulary(text):
    want = R.tokenize(HAND, text)
    assert E.tokenize_host(HAND, text) == want


def test_tokenize_known_answers():
    assert E.tokenize_host(HAND, b"abcab") == [2, 1]
    assert E.tokenize_host(HAND, b" abab") == [3, 1]
    assert E.tokenize_host(HAND, b"ab'll a") == [1, 5, 8, 0]
    assert E.tokenize_host(HAND, b"121 2") == [7, 6, 8]
    assert E.tokenize_host(HAND, b"") == []
    assert R.pieces(b"it's 42 !? x") == [b"it", b"'s", b" 42", b" !?", b" x"]


def test_tokenize_cap_one_too_small():
    n = len(R.tokenize(HAND, b"abcab a"))
    assert len(E.tokenize_host(HAND, b"abcab a", cap=n)) == n
    with pytest.raises(E.WhisperError) as ei:
        E.tokenize_host(HAND, b"abcab a", cap=n - 1)
    assert ei.value.code == E.OHW_E_INVALID_ARG and f"{n} tokens" in str(ei.value)


def test_tokenize_synthetic_vocabulary():
    vocab = modelfile.synthetic_vocab(synth.PRESETS["micro"])
    for text in (b" w5 w50256 w12", b"w7 w1'd", b" w0  w1", b"hello 123", b""):
        assert E.tokenize_host(vocab, text) == R.tokenize(vocab, text), text
    # letters and digits are separate pieces, so " w5" is never looked up whole: " w" gives " " (220), w and 5 start no entry
    assert E.tokenize_host(vocab, b" w5 w123") == [220, 220]


@pytest.mark.parametrize("n", [0, 1, 223, 224, 300])
def test_prompt_clip(n):
    toks = list(range(1000, 1000 + n))
    got = E.prompt_clip(toks, 448)
    assert got == R.clip(toks, 448) == toks[max(0, n - 223):]
    assert len(got) == min(n, 223)


LENS = [[0, 2, 8, 9, 224], [0], [224], [1, 2, 3, 7, 8, 9, 15, 16, 17], [5, 0, 12]]


@pytest.mark.parametrize("lens", LENS)
def test_chunk_plan_never_reads_a_surplus_position(lens):
    """positions at or past a window's length that the chunks write ([eot] rows) are overwritten by the decode before any
    query reads them, and no position reaches n_text_ctx (448, 4 prompt tokens, the largest n_max the entries allow)"""
    n_steps = 448 - 4 - max(lens) - 1
    assert R.simulate(lens, 4, n_steps, 448) == []
    plan = R.chunk_plan(lens, None, -1, -2)
    assert len(plan) == -(-max(lens) // 8)
    for n_past, fed, done in plan:
        assert n_past + 8 <= 224 + 7 and n_past % 8 == 0
        for b, n in enumerate(lens):
            assert done[b] == (1 if n_past >= n else 0)
            assert fed[b] == [(-1 if p == 0 else p) if p < n else -2 for p in range(n_past, n_past + 8)]


def test_cache_model_catches_a_decode_that_starts_one_position_late():
    """the model is not vacuous: a decode that skips a position reads the surplus row left there"""
    lens = [3]
    bad = []
    cell = {}
    for p in range(8):
        cell[p] = "ctx" if p < 3 else "pad"
    for p in (4,):                      # the prompt token lands on position 4 instead of 3
        cell[p] = "own"
        bad += [k for k in range(p + 1) if cell.get(k) in (None, "pad")]
    assert bad == [3]
    assert R.simulate(lens, 4, 10, 448) == []
    assert any(v[0] == "position" for v in R.simulate([224], 4, 448, 448))


def test_chunk_plan_with_inactive_windows():
    plan = R.chunk_plan([20, 9, 3], None, -1, -2, active=[0, 1, 1])
    assert len(plan) == 2                                   # the inactive window's 20 positions do not extend the loop
    assert [d for _, _, d in plan] == [[1, 0, 0], [1, 0, 1]]
