"""Word-timestamp alignment, the host twins (no GPU): ohw_dtw_host is bit-defined and must equal the float32 reference
exactly; ohw_align_reduce_host against float64 within the bound derived in align_ref.reduce_bound."""
import numpy as np
import pytest

import align_ref as R

NS = [1, 2, 9, 40]
KS = [1, 2, 7, 65]


@pytest.fixture(scope="module")
def E():
    from openhush_amd import engine
    assert hasattr(engine.lib(), "ohw_dtw_host") and hasattr(engine.lib(), "ohw_align_reduce_host")
    return engine


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("k", KS)
def test_dtw_host_equals_the_reference_exactly(E, n, k):
    rng = np.random.default_rng(100 * n + k)
    for trial in range(3):
        m = rng.standard_normal((n, k)).astype(np.float32)
        want, path = R.dtw_ref(m)
        got = E.dtw(m)
        assert R.starts_wrong(want, got) == 0, (n, k, trial, want.tolist(), got.tolist())
        # a path: starts at (0, 0), ends at (n - 1, k - 1), every step one of the three moves
        assert path[0] == (0, 0) and path[-1] == (n - 1, k - 1)
        assert all((b[0] - a[0], b[1] - a[1]) in ((1, 1), (1, 0), (0, 1)) for a, b in zip(path, path[1:]))
        assert np.all(np.diff(got) >= 0) and got[0] == 0 and got[-1] <= k - 1


@pytest.mark.parametrize("n", [1, 2, 9, 40])
def test_dtw_host_on_the_planted_diagonal(E, n):
    m, want = R.planted_diagonal(n)
    assert R.starts_wrong(want, R.dtw_ref(m)[0]) == 0
    assert R.starts_wrong(want, E.dtw(m)) == 0


@pytest.mark.parametrize("n,k", [(1, 1), (2, 7), (9, 9), (9, 2), (40, 65), (7, 40)])
def test_dtw_host_on_all_equal_entries_follows_the_tie_rule(E, n, k):
    # no strict minimum anywhere except against the infinite border: the rule's last branch (trace 2) decides
    for v in (0.0, 1.0, -0.375):
        m = np.full((n, k), v, dtype=np.float32)
        want, _ = R.dtw_ref(m)
        assert R.starts_wrong(want, E.dtw(m)) == 0, (n, k, v)


def test_the_reference_flags_a_path_shifted_by_one_key(E):
    # guard against a comparison that cannot fail: one key off on the planted diagonal is caught, by index and by cost
    m, want = R.planted_diagonal(9)
    got = E.dtw(m)
    assert R.starts_wrong(want, got) == 0
    shifted = np.minimum(got + 1, m.shape[1] - 1)
    assert R.starts_wrong(want, shifted) == 9
    one_off = got.copy()
    one_off[4] += 1
    assert R.starts_wrong(want, one_off) == 1
    _, path = R.dtw_ref(m)
    best = R.optimum64(m)
    assert R.path_cost64(m, path) == best == -18.0
    moved = [(r, min(t + 1, m.shape[1] - 1)) for r, t in path]
    assert R.path_cost64(m, moved) >= best + 8.0        # every row loses one of its two ones (the last cell cannot move)


def _probs(rng, A, n_all, n_keys, peaked):
    lg = rng.standard_normal((A, n_all, n_keys)) * (4.0 if peaked else 1.0)
    e = np.exp(lg - lg.max(axis=2, keepdims=True))
    return (e / e.sum(axis=2, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("n_keys", [1, 3, 7, 64])
@pytest.mark.parametrize("A,n_all,n_prompt", [(1, 5, 4), (2, 12, 4), (3, 30, 2)])
def test_reduce_host_against_float64(E, n_keys, A, n_all, n_prompt):
    rng = np.random.default_rng(n_keys * 1000 + A)
    p = _probs(rng, A, n_all, n_keys, peaked=(A == 2))
    if n_keys >= 3:
        p[:, :, 1] = 0.25          # a column with std == 0 (n * 0.25 and its mean are exact): z must be exactly 0 there
        p[0, :, 2] = 0.0
    got = E.align_reduce(p, n_prompt)
    want = R.reduce_ref(p, n_prompt)
    bound = R.reduce_bound(p, n_prompt)
    assert got.shape == want.shape == (n_all - n_prompt, n_keys)
    err = np.abs(got.astype(np.float64) - want)
    print(f"reduce host n_keys {n_keys} A {A} n_all {n_all}: max err {err.max():.3g}, smallest bound {bound.min():.3g}, largest {bound.max():.3g}")
    assert np.isfinite(bound).all()
    assert (err <= bound).all(), (float(err.max()), float(bound.min()))
    if n_keys == 1:
        # softmax over one key is 1 in every row: std == 0 everywhere, m is exactly 0
        assert not got.any()


def test_reduce_host_median_is_a_selection(E):
    # one head: every m value is one of the head's z values of that row (a median selects, it never averages)
    rng = np.random.default_rng(5)
    p = _probs(rng, 1, 20, 33, peaked=True)
    got = E.align_reduce(p, 0)
    p64 = p.astype(np.float64)
    z = (p64 - p64.mean(axis=1, keepdims=True)) / p64.std(axis=1, keepdims=True)
    ref = R.median7(z)[0]
    pad = np.pad(z[0], [(0, 0), (3, 3)], mode="reflect")
    for r in range(20):
        for t in range(33):
            win = pad[r, t:t + 7]
            pick = int(np.argmin(np.abs(win - ref[r, t])))
            assert abs(float(got[r, t]) - win[pick]) <= R.reduce_bound(p, 0)[r, t]


def test_host_twins_refuse_bad_arguments(E):
    with pytest.raises(E.WhisperError):
        E.dtw(np.zeros((0, 4), np.float32))
    with pytest.raises(E.WhisperError):
        E.align_reduce(np.zeros((2, 4, 3), np.float32), 4)      # nothing left behind the prompt
    with pytest.raises(E.WhisperError):
        E.align_reduce(np.zeros((33, 5, 3), np.float32), 1)     # more than OHW_ALIGN_MAX_HEADS heads


# ---------------------------------------------------------------------------------------------------------------------------
# the host rules of the engine's words and segments
# ---------------------------------------------------------------------------------------------------------------------------
def test_word_rule_on_byte_strings(E):
    # "é" = c3 a9 split across two tokens: the token in between the halves cannot start a word even though it begins with a space
    toks = [b" caf", b"\xc3", b"\xa9", b" au", b" l", b"ait", b",", b" \xe2\x82", b" x", b"\xac", b" y"]
    want = [True, False, False, True, True, False, False, True, False, False, False]
    #                                                               ^ " x" follows e2 82 (incomplete): no word start;
    #        "\xac" then completes nothing that begins with a space; " y" follows 82 20 78 ac: the byte in front, ac, is a
    #        continuation byte whose lead (78 = "x") takes none, so the bytes in front do not end on a complete sequence
    assert E.word_starts(toks) == want
    assert E.word_starts([b"no", b"space", b" here"]) == [True, False, True]        # the first token of a window always starts one
    assert E.word_starts([]) == []
    assert E.word_starts([b" a", b"", b" b"]) == [True, False, True]
    # four-byte character split 2 + 2
    assert E.word_starts([b" \xf0\x9f", b" z", b"\x98\x80", b" ok"]) == [True, False, False, False]
    assert E.word_starts([b" \xf0\x9f\x98\x80", b" ok"]) == [True, True]


def test_segment_rule_on_token_lists(E):
    tok = E.SpecialTokens()
    tok.eot, tok.timestamp_begin = 50257, 50364
    ts = lambda s: 50364 + int(round(s / 0.02))
    f32 = lambda x: float(np.float32(x))
    # closed segments, back-to-back timestamps, an open tail
    t = [ts(0.0), 11, 12, ts(2.0), ts(2.0), 13, ts(3.5), ts(4.0), 14, 15]
    got = E.segments_host(t, tok, 30.0, 42.5)
    want = [(1, 3, 30.0, 32.0), (5, 6, 32.0, f32(np.float32(30.0) + np.float32(175) * np.float32(0.02))), (8, 10, 34.0, 42.5)]
    assert [(a, b) for a, b, _, _ in got] == [(a, b) for a, b, _, _ in want]
    for g, w in zip(got, want):
        assert abs(g[2] - w[2]) < 1e-5 and abs(g[3] - w[3]) < 1e-5, (g, w)
    # text in front of the first timestamp starts at the window's offset; specials between eot and timestamp_begin carry no text
    assert E.segments_host([7, 8, ts(1.0)], tok, 60.0, 90.0) == [(0, 2, 60.0, 61.0)]
    assert E.segments_host([ts(0.0), 50258, 50300, ts(1.0)], tok, 0.0, 30.0) == []
    assert E.segments_host([ts(0.0), ts(1.0), ts(1.0)], tok, 0.0, 30.0) == []
    assert E.segments_host([], tok, 0.0, 30.0) == []
    # an open tail ends at the end the caller gives: the earlier of the window's end and the recording's end
    assert E.segments_host([ts(28.0), 9], tok, 30.0, 70.0 - 0.0) [0][3] == 70.0
