"""Best-of sampling, the parts that need no GPU: the pick (ohw_best_of_pick_host, the function the engine's rung calls) against
the float64 restatement in best_of_ref.py on crafted candidate sets with no near-ties, the generator rule (candidate j draws
from std::mt19937(j)), the batch-size rule, and the argument errors of the host entries.  An engine needs a device, so the
engine setters' own errors are checked in test_gpu_engine_best_of.py."""
import ctypes as C

import numpy as np
import pytest

import best_of_ref
from openhush_amd import engine as E


def _policy(entropy_thold=2.4):
    q = E.DecodePolicy()
    E.lib().ohw_default_decode_policy(C.byref(q))
    q.entropy_thold = entropy_thold
    return q


def _ev(avg, ent=3.0, failed=0):
    return E.SeqEval(10, 10, 9, 3000, failed, 0 if failed else 1, avg, ent)


def _as_dicts(evs):
    return [{"failed": e.failed, "entropy": e.entropy, "avg_logprob": e.avg_logprob} for e in evs]


CASES = {
    # name: (candidates, the pick written down by hand)
    "winner is not candidate 0": ([_ev(-0.9), _ev(-0.7), _ev(-0.3), _ev(-0.5)], 2),
    "best average knocked out by entropy": ([_ev(-0.9), _ev(-0.2, ent=1.0), _ev(-0.6)], 2),
    "best knocked out by failed": ([_ev(-0.9), _ev(-0.8), _ev(-0.1, failed=1)], 1),
    "all out: candidate 0": ([_ev(-0.9, failed=1), _ev(-0.2, ent=0.5), _ev(-0.1, failed=1), _ev(-0.3, ent=2.0), _ev(-0.4, failed=1)], 0),
    "exact equality: lowest j": ([_ev(-0.75), _ev(-0.5), _ev(-0.5), _ev(-0.5)], 1),
    "one candidate": ([_ev(-2.0, failed=1)], 0),
    "entropy exactly at the threshold stays in": ([_ev(-0.9), _ev(-0.4, ent=2.4000000953674316)], 1),
    "-inf average (no result) loses to any finite one": ([_ev(-np.inf), _ev(-5.0)], 1),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_pick_equals_the_restatement(name):
    evs, want = CASES[name]
    q = _policy()
    got = E.best_of_pick_host(evs, q)
    ref = best_of_ref.pick(_as_dicts(evs), float(q.entropy_thold))
    assert got == ref == want, (name, got, ref, want)


def test_pick_on_random_sets_without_near_ties():
    """400 random sets: averages on a 0.05 grid with distinct values or exact repeats, entropies at least 0.1 from the threshold"""
    rng = np.random.default_rng(3)
    q = _policy()
    kept_nonzero = all_out = 0
    for _ in range(400):
        n = int(rng.integers(1, 6))
        evs = [_ev(float(np.float32(-0.05 * int(rng.integers(1, 40)))), ent=float(rng.choice([1.0, 2.3, 2.5, 3.4])), failed=int(rng.random() < 0.25))
               for _ in range(n)]
        got = E.best_of_pick_host(evs, q)
        assert got == best_of_ref.pick(_as_dicts(evs), float(q.entropy_thold))
        kept_nonzero += got != 0
        all_out += all(best_of_ref.is_out(c, float(q.entropy_thold)) for c in _as_dicts(evs))
    assert kept_nonzero > 50 and all_out > 10


def test_the_restatement_notices_a_wrong_pick():
    """swap two candidates and keep the old index: the restatement must say no"""
    evs, want = CASES["winner is not candidate 0"]
    d = _as_dicts(evs)
    thold = 2.4
    assert best_of_ref.check_pick(d, thold, want)
    swapped = list(d)
    swapped[want], swapped[0] = swapped[0], swapped[want]
    assert not best_of_ref.check_pick(swapped, thold, want)
    assert best_of_ref.check_pick(swapped, thold, 0)
    for wrong in (0, 1, 3, -1, 4):
        assert not best_of_ref.check_pick(d, thold, wrong)
    # and the library's pick follows the swap
    q = _policy()
    assert E.best_of_pick_host([evs[want]] + evs[1:want] + [evs[0]] + evs[want + 1:], q) == 0


def test_pick_argument_errors():
    q = _policy()
    L = E.lib()
    arr = (E.SeqEval * 6)(*[_ev(-0.5) for _ in range(6)])
    kept = np.zeros(1, np.int32)
    for n in (0, 6, -1):
        assert L.ohw_best_of_pick_host(arr, n, C.byref(q), E._ip(kept)) == E.OHW_E_INVALID_ARG
    assert L.ohw_best_of_pick_host(None, 2, C.byref(q), E._ip(kept)) == E.OHW_E_INVALID_ARG
    assert L.ohw_best_of_pick_host(arr, 2, None, E._ip(kept)) == E.OHW_E_INVALID_ARG
    assert L.ohw_best_of_pick_host(arr, 2, C.byref(q), None) == E.OHW_E_INVALID_ARG
    # the engine entries refuse a null engine before anything else
    assert L.ohw_engine_set_best_of(None, 2) == E.OHW_E_INVALID_ARG
    assert L.ohw_pool_set_best_of(None, 2) == E.OHW_E_INVALID_ARG
    p, n = C.POINTER(C.c_int32)(), C.c_int(0)
    assert L.ohw_engine_last_candidates(None, C.byref(p), C.byref(n)) == E.OHW_E_INVALID_ARG


def _std_mt19937_canonical(seed: int, n: int) -> np.ndarray:
    """n draws of std::generate_canonical<double, 53> over std::mt19937(seed), from numpy's MT19937 in the state
    init_genrand(seed) leaves it in (RandomState's legacy integer seeding; MT19937(seed) itself seeds through SeedSequence)"""
    st = np.random.RandomState(seed).get_state()
    bg = np.random.MT19937()
    bg.state = {"bit_generator": "MT19937", "state": {"key": st[1], "pos": st[2]}}
    raw = bg.random_raw(2 * n).astype(np.float64)
    x = (raw[0::2] + raw[1::2] * 4294967296.0) / 18446744073709551616.0
    return np.where(x < 1.0, x, np.nextafter(1.0, 0.0))


def test_candidate_j_draws_from_mt19937_seeded_with_j():
    from oracle import oracle
    from test_rng_draws_cpu import _mt_canonical
    seen = set()
    for j in range(5):
        u = E.HostRng(j).uniforms(700)               # past one twist of the state (312 draws)
        assert u.tobytes() == _std_mt19937_canonical(j, 700).tobytes(), j
        ref = oracle.MT19937(j)
        assert u[:50].tobytes() == np.array([_mt_canonical(ref) for _ in range(50)], np.float64).tobytes(), j
        seen.add(u[:4].tobytes())
    assert len(seen) == 5                             # five different streams
    # a candidate's generator moves on by its own pass's draws only
    a, b = E.HostRng(3), E.HostRng(3)
    a.discard_draws(17)
    assert a.uniforms(5).tobytes() == b.uniforms(22)[17:].tobytes()


def test_batch_size_rule():
    for mb in (1, 2, 3, 5, 6, 15, 16, 32, 96):
        for k in (0, 2, 3, 4, 5):
            for n in (1, 2, 3, 4, 5):
                want = mb // max(n, k, 1)
                if want < 1:
                    with pytest.raises(E.WhisperError):
                        E.batch_windows_host(mb, k, n)
                else:
                    assert E.batch_windows_host(mb, k, n) == want, (mb, k, n)
    # best_of 1 and no beam: the batch as it always was
    assert E.batch_windows_host(32) == 32 and E.batch_windows_host(32, 5, 1) == 6 and E.batch_windows_host(32, 2, 5) == 6
    for bad in ((0, 0, 1), (8, 1, 1), (8, 6, 1), (8, 0, 0), (8, 0, 6), (8, -1, 1)):
        with pytest.raises(E.WhisperError):
            E.batch_windows_host(*bad)
