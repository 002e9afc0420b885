"""Confidence scores without a GPU: ohw_token_score_host and ohw_word_probs_host against the float64 restatement of
tests/score_ref.py, and the proof that score_ref.compare() - the comparison tests/test_gpu_token_score.py makes - flags every
injected fault on the shared cases."""
import numpy as np
import pytest

import score_ref as R

P = 4
N_ALL = [0, P, P + 1, 8, 9, 16]
CASES = [(1003, 900, 1012), (51866, 50257, 51880)]


@pytest.fixture(scope="module")
def E():
    from openhush_amd import engine
    assert hasattr(engine.lib(), "ohw_token_score_host") and hasattr(engine.lib(), "ohw_word_probs_host")
    return engine


def _host_scores(E, case):
    """what the kernel's host twin gives for the case, laid out as ohw_dbg_token_score lays its result out"""
    want, written = R.expected(case)
    out = R.as_device(want, np.zeros_like(written))
    body = out.reshape(written.shape)
    for b, e in np.argwhere(written):
        m = b * 8 + (e + case["n_prompt"] - 1 - case["row0"])
        s = E.token_score_host(case["logits"][m], case["eot"], int(case["targets"][m]), n_vocab=case["n_vocab"])
        for f in R.FIELDS:
            body[f][b, e] = s[f]
    return out


def test_bounds_are_printed():
    R.print_bounds()
    assert R.n_t(1003) == 4 and R.n_t(51866) == 204
    assert 1.01 * R.U * 6 * (R.n_t(51866) + 10) < 1e-4          # the bound is tight enough to see one misplaced column of a planted row


@pytest.mark.parametrize("row0", [0, 8])
@pytest.mark.parametrize("n_vocab,eot,ld", CASES)
def test_host_rule_equals_the_restatement(E, n_vocab, eot, ld, row0):
    case = R.make_case(n_vocab, eot, ld, N_ALL, row0)
    bad, worst = R.compare(case, _host_scores(E, case))
    print(f"token_score_host {n_vocab} columns row0 {row0}: worst lse error / bound {worst:.3f}")
    assert not bad, bad[:4]


def test_host_rule_ignores_the_padding_and_refuses_nonsense(E):
    x = (3.0 * np.random.default_rng(1).standard_normal(1012)).astype(np.float32)
    a = E.token_score_host(x, 900, 5, n_vocab=1003)
    x[1003:] = R.POISON
    b = E.token_score_host(x, 900, 5, n_vocab=1003)
    assert a.tobytes() == b.tobytes()
    L = E.lib()
    assert L.ohw_token_score_host(None, 10, 5, 0, None) == E.OHW_E_INVALID_ARG
    assert L.ohw_word_probs_host(None, None, -1, None) == E.OHW_E_INVALID_ARG


@pytest.mark.parametrize("fault", R.FAULTS)
def test_the_comparison_flags_every_injected_fault(fault):
    flagged = 0
    for n_vocab, eot, ld in CASES[:1] if fault != "eot_in_lse_text" else CASES:
        for row0 in (0, 8):
            case = R.make_case(n_vocab, eot, ld, N_ALL, row0)
            want, written = R.expected(case, fault=fault)
            bad, _ = R.compare(case, R.as_device(want, written, guard=2), guard=2)
            flagged += bool(bad)
    assert flagged, fault
    # and the clean restatement passes its own comparison, guards included
    case = R.make_case(*CASES[0], N_ALL, 0)
    assert R.compare(case, R.as_device(*R.expected(case), guard=2), guard=2)[0] == []


def test_a_guard_entry_written_is_flagged():
    case = R.make_case(*CASES[0], N_ALL, 0)
    dev = R.as_device(*R.expected(case), guard=2)
    dev["top_id"][-1] = 3
    assert R.compare(case, dev, guard=2)[0]


def test_token_prob_host_is_the_two_subtractions(E):
    s = np.zeros(1, E.TOKEN_SCORE_DTYPE)[0]
    s["logit"], s["lse_text"], s["lse_all"], s["top_id"], s["top_logit"] = 1.5, 10.25, 10.375, 7, 9.0
    lt, la, tt = E.token_prob_host(s)
    assert lt == np.float32(1.5) - np.float32(10.25) and la == np.float32(1.5) - np.float32(10.375) and tt == np.float32(9.0) - np.float32(10.25)


def test_word_probs_host_is_the_float64_mean(E):
    rng = np.random.default_rng(3)
    for n in (0, 1, 2, 7, 60):
        lp = (-np.abs(rng.standard_normal(n)) * 2).astype(np.float32)
        starts = (rng.random(n) < 0.4).astype(np.int32)
        got = E.word_probs_host(lp, starts)
        want = R.word_probs(lp, starts) if n else np.zeros(0)
        assert got.shape == want.shape
        # one rounding of the double mean; libm's exp and numpy's may differ in the double's last place: one float ulp at most
        assert (np.abs(got.astype(np.float64) - want) <= np.spacing(want.astype(np.float32)).astype(np.float64)).all(), (n, got, want)
    # token 0 opens a word whatever starts[0] says
    assert E.word_probs_host([-0.5, -0.25], [0, 0]).tolist() == E.word_probs_host([-0.5, -0.25], [1, 0]).tolist()
