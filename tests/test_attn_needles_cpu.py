"""The needle construction (tests/attn_needles.py) and its checker, without a GPU.

Each fault an attention kernel could have is applied to the float64 REFERENCE, never to a kernel, and the comparison the GPU
tests use must flag it with an error of at least 8 times the (larger, bf16) tolerance.  The construction's own guarantees - the
needle weights, pairs that straddle the kernel's units, the untiling index - are asserted at every shape the GPU tests use.
"""
import numpy as np
import pytest

import attn_needles as A

FLAG = 8 * A.TOL[0]


def _flagged(c, ref, **fault):
    return A.worst_error(A.reference(c, **fault), ref)


def _all_cases():
    for family, cases in (("encoder", A.ENCODER_CASES), ("cross", A.CROSS_CASES), ("self", A.SELF_CASES)):
        for name in cases:
            yield family, name


@pytest.mark.parametrize("family,name", list(_all_cases()))
def test_construction_guarantees(family, name):
    worst = {}
    for pattern in A.PATTERNS:
        c, ref, w = A.make(family, name, pattern)
        worst[pattern] = 1.0 - w.min()
        assert w.min() >= A.MIN_WEIGHT[pattern], (pattern, w.min())
        assert np.abs(ref).max() <= 1.0 + 1e-9                  # no allowed key is poison
        assert (c.needle < c.n_keys[:, None]).all() and (c.needle2 < c.n_keys[:, None]).all()
        # exactly representable in bf16 (8 significant bits) and f16: small integers, and multiples of 2^-6 below 1
        assert set(np.unique(np.abs(c.q))) <= {0.0, A.GAIN[pattern]}
        assert set(np.unique(np.abs(c.K))) <= {1.0, 2.0}
        live = c.V[np.abs(c.V) < 50]
        assert (live * 64 == np.round(live * 64)).all() and np.abs(live).max() <= 1.0
        if pattern != "pair":
            assert (c.needle2 == c.needle).all()
            continue
        # a pair straddles the first partition of the positions that has more than one unit among the row's keys
        for r in range(c.R):
            n = int(c.n_keys[r])
            part = next((u for u in c.units if len(np.unique(u[:n])) > 1), None)
            for h in range(c.H):
                a, b = c.needle[r, h], c.needle2[r, h]
                assert (a != b) == (n > 1)
                if part is not None:
                    assert part[a] != part[b], (r, h, a, b)
    print(f"needle weights {family} {name}: 1 - w <= " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))


@pytest.mark.parametrize("M", [1, 2, 3, 4, 6, 8, 9, 10, 12, 16, 17, 20, 64])
def test_untiling_index_is_a_permutation(M):
    d = 128
    idx = A.act_tiled_index(M, d).reshape(-1)
    assert len(np.unique(idx)) == M * d and idx.min() >= 0 and idx.max() < A.tiled_elems(M, d)
    if M % 16 == 0:
        assert (np.sort(idx) == np.arange(M * d)).all()
    # element (m, k): tile m / 16, k-block k / 32, lane m % 16 + 16 * ((k % 32) / 8), slot k % 8
    m, k = M - 1, 77
    assert A.act_tiled_index(M, d)[m, k] == (((m // 16) * 4 + 2) * 64 + m % 16 + 16 * 1) * 8 + 5


FAULT_CASES = [("encoder", "T65"), ("encoder", "var"), ("cross", "plain_t63_m17"), ("cross", "split_t1500_m17"), ("cross", "var_rows2"),
               ("cross", "group_split_t250"), ("self", "plain_n1"), ("self", "plain_n8"), ("self", "slots_n2")]


@pytest.mark.parametrize("pattern", A.PATTERNS)
@pytest.mark.parametrize("family,name", FAULT_CASES)
def test_dropped_last_key_is_flagged(family, name, pattern):
    c, ref, _ = A.make(family, name, pattern)
    assert _flagged(c, ref, edit=lambda r, pos: pos[:-1] if len(pos) > 1 else pos) >= FLAG


@pytest.mark.parametrize("pattern", A.PATTERNS)
@pytest.mark.parametrize("z", range(8))
def test_dropped_first_key_of_a_slice_is_flagged(z, pattern):
    c, ref, _ = A.make("cross", "split_t1500_m17", pattern)
    sl = A.xattn_slice_of(1500, 8)
    assert sl.max() == 7 and (sl == 7).sum() == 1500 - 7 * 24 * 8          # 24 groups of 8 keys per slice, the last one short
    first = int(np.nonzero(sl == z)[0][0])
    assert _flagged(c, ref, edit=lambda r, pos: pos[pos != first]) >= FLAG


@pytest.mark.parametrize("pattern", A.PATTERNS)
@pytest.mark.parametrize("family,name", [("encoder", "var"), ("cross", "var_plain"), ("cross", "var_rows3")])
def test_key_past_the_window_length_is_flagged(family, name, pattern):
    c, ref, _ = A.make(family, name, pattern)
    P = c.K.shape[2]
    assert _flagged(c, ref, edit=lambda r, pos: np.append(pos, len(pos)) if len(pos) < P else pos) >= FLAG


@pytest.mark.parametrize("pattern", A.PATTERNS)
@pytest.mark.parametrize("name", list(A.SELF_CASES))
def test_causal_off_by_one_is_flagged(name, pattern):
    """key n_past + i + 1: poison behind a window's last new token, the next token's twin of the needle for the others"""
    c, ref, _ = A.make("self", name, pattern)
    got = A.reference(c, edit=lambda r, pos: np.append(pos, len(pos)) if len(pos) < A.N_CTX else pos)
    assert A.worst_error(got, ref) >= FLAG
    if c.table is None:
        # plain: every new token is flagged by itself, not only one of the launch
        for r in range(c.R):
            if c.n_keys[r] < A.N_CTX:
                assert np.abs(got[r] - ref[r]).max() >= FLAG, r


@pytest.mark.parametrize("pattern", A.PATTERNS)
@pytest.mark.parametrize("name", ["slots_n1", "slots_n2", "slots_n8"])
def test_swapped_slot_entries_are_flagged(name, pattern):
    c, ref, _ = A.make("self", name, pattern)
    slab = c.slab.copy()
    for r in range(c.R):
        a = c.needle[r, 0]
        other = [j for j in range(int(c.n_keys[r])) if slab[r, j] != slab[r, a]]
        if other:                                                           # the needle's entry and one that names another row
            slab[r, a], slab[r, other[0]] = slab[r, other[0]], slab[r, a]
    assert _flagged(c, ref, slab=slab) >= FLAG


@pytest.mark.parametrize("pattern", A.PATTERNS)
@pytest.mark.parametrize("family,name", FAULT_CASES)
def test_neighbouring_window_and_swapped_heads_are_flagged(family, name, pattern):
    c, ref, _ = A.make(family, name, pattern)
    S = c.K.shape[0]
    assert _flagged(c, ref, slab=(c.slab + 1) % S) >= FLAG                  # window b + 1's K / V for window b
    assert _flagged(c, ref, head_map=[1, 0]) >= FLAG


@pytest.mark.parametrize("family,name", FAULT_CASES)
def test_missed_rescale_of_a_pair_is_flagged(family, name):
    """the two halves of a pair weighted 1 : 0.5 instead of 1 : 1"""
    c, ref, _ = A.make(family, name, "pair")
    assert (c.needle2 != c.needle).any()

    def scale(r, h, pos, p):
        p = p.copy()
        if c.needle2[r, h] != c.needle[r, h]:
            p[pos == c.needle2[r, h]] *= 0.5
        return p
    assert _flagged(c, ref, scale=scale) >= FLAG
