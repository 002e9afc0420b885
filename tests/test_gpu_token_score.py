"""token_score_kernel alone, through ohw_dbg_token_score: the entries it leaves in sentinel-filled, guarded output must equal the
float64 restatement of tests/score_ref.py - selections word for word, the two log-sum-exp values inside the bound score_ref derives
from the reduction order - and everything the contract does not name must still hold the sentinel.  The logits rows carry poison in
their padding columns and sit between two NaN guard rows on the device."""
import numpy as np
import pytest

from openhush_amd import synth

import score_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

P, CAP, GUARD = 4, 16, 3
N_ALL = [0, P, P + 1, 8, 9, 16]
SIZES = [(1003, 900, 1012), (51866, 50257, 51880)]


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from openhush_amd import engine
    assert hasattr(engine.lib(), "ohw_dbg_token_score")
    return engine


@pytest.fixture(scope="module")
def st(E):
    ctx = E.Context.synthetic(synth.PRESETS["nano"].as_list(), 1234, 0, 1)
    s = E.State(ctx, 1)
    yield s
    s.close()


def _n_all(batch, rot):
    return [N_ALL[(b + rot) % len(N_ALL)] for b in range(batch)]


def _run(E, st, case):
    got = st.dbg_token_score(case["logits"], case["n_vocab"], case["eot"], case["targets"], case["n_all"], case["row0"], case["n_prompt"],
                             case["cap"], guard=GUARD)
    bad, worst = R.compare(case, got, guard=GUARD)
    return got, bad, worst


@pytest.mark.parametrize("row0", [0, 8])
@pytest.mark.parametrize("batch", [1, 3, 13])
@pytest.mark.parametrize("n_vocab,eot,ld", SIZES)
def test_rows_against_the_restatement(E, st, n_vocab, eot, ld, batch, row0):
    assert E.OHW_DBG_SENTINEL_I32 == R.SENT_I and E.OHW_DBG_SENTINEL_F32 == float(R.SENT_F)
    # one window sees every n_all in turn; three windows in two rotations; thirteen hold every value at least twice
    for rot in {1: range(6), 3: (0, 3), 13: (0,)}[batch]:
        case = R.make_case(n_vocab, eot, ld, _n_all(batch, rot), row0, n_prompt=P, cap=CAP, seed=rot)
        got, bad, worst = _run(E, st, case)
        n_written = int(R.expected(case)[1].sum())
        print(f"token_score {n_vocab} columns batch {batch} row0 {row0} n_all {case['n_all'].tolist()}: {n_written} entries, "
              f"worst lse error / bound {worst:.3f}")
        assert not bad, bad[:4]


def test_the_cases_plant_what_they_claim():
    """over the written rows of the GPU cases: a maximum on column 0, eot - 1, eot, n_vocab - 1 and on both sides of a thread, a wave
    and a stride seam; ties between text columns; rows whose largest value is not a text column"""
    for n_vocab, eot, ld in SIZES:
        top_cols, tgt_cols, ties, non_text = set(), set(), 0, 0
        for batch, rots in ((1, range(6)), (3, (0, 3)), (13, (0,))):
            for rot in rots:
                for row0 in (0, 8):
                    case = R.make_case(n_vocab, eot, ld, _n_all(batch, rot), row0, n_prompt=P, cap=CAP, seed=rot)
                    _, written = R.expected(case)
                    for b, e in np.argwhere(written):
                        x = case["logits"][b * 8 + e + P - 1 - row0, :n_vocab]
                        top_cols.add(int(np.argmax(x)))
                        tgt_cols.add(int(case["targets"][b * 8 + e + P - 1 - row0]))
                        ties += int((x[:eot] == x[:eot].max()).sum() > 1)
                        non_text += int(np.argmax(x) >= eot)
        need = {0, eot - 1, eot, n_vocab - 1, 3, 4, 255, 256, 1023, 1024} & set(R.seam_columns(n_vocab, eot))
        assert need <= top_cols, (n_vocab, sorted(need - top_cols))
        assert {0, eot - 1, eot, n_vocab - 1} <= tgt_cols, (n_vocab, sorted(tgt_cols))
        assert ties >= 4 and non_text >= 4, (n_vocab, ties, non_text)


@pytest.mark.parametrize("n_vocab,eot,ld", SIZES)
def test_a_rows_words_do_not_depend_on_its_slot_or_the_batch(E, st, n_vocab, eot, ld):
    small = R.make_case(n_vocab, eot, ld, [16, 16, 16], 0, n_prompt=P, cap=CAP, seed=9)
    big = R.make_case(n_vocab, eot, ld, [16] * 13, 0, n_prompt=P, cap=CAP, seed=10)
    # rows 3 .. 7 of window 2 of the small batch become rows 3 .. 7 of window 11 of the big one
    big["logits"][11 * 8:12 * 8] = small["logits"][2 * 8:3 * 8]
    big["targets"][11 * 8:12 * 8] = small["targets"][2 * 8:3 * 8]
    a, bad_a, _ = _run(E, st, small)
    b, bad_b, _ = _run(E, st, big)
    assert not bad_a and not bad_b, (bad_a[:2], bad_b[:2])
    ea = a[GUARD:GUARD + 3 * CAP].reshape(3, CAP)[2]
    eb = b[GUARD:GUARD + 13 * CAP].reshape(13, CAP)[11]
    assert ea[:5].tobytes() == eb[:5].tobytes() and (ea["top_id"][:5] != R.SENT_I).all()


def test_refusals_launch_nothing(E, st):
    case = R.make_case(1003, 900, 1012, [9], 0, n_prompt=P, cap=CAP)

    def rc(**kw):
        a = dict(logits=case["logits"], n_vocab=1003, eot=900, targets=case["targets"], n_all=case["n_all"], row0=0, n_prompt=P, cap=CAP)
        a.update(kw)
        try:
            st.dbg_token_score(a["logits"], a["n_vocab"], a["eot"], a["targets"], a["n_all"], a["row0"], a["n_prompt"], a["cap"])
        except E.WhisperError as e:
            return e.code
        return 0

    bad_t = case["targets"].copy()
    bad_t[3] = 1003
    assert rc(targets=bad_t) == E.OHW_E_INVALID_ARG
    assert rc(logits=case["logits"][:, :1010]) == E.OHW_E_INVALID_ARG           # ld % 4 != 0
    assert rc(n_vocab=1013) == E.OHW_E_INVALID_ARG                               # ld < n_vocab
    assert rc(n_prompt=0) == E.OHW_E_INVALID_ARG and rc(cap=0) == E.OHW_E_INVALID_ARG and rc(row0=-1) == E.OHW_E_INVALID_ARG
    assert rc() == 0
