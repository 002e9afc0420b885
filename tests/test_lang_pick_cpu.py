"""ohw_lang_pick_host, the host definition of the device language pick, against numpy on crafted rows (no GPU)."""
import numpy as np
import pytest

from openhush_amd import synth

from lang_rows import SOT, crafted_rows, numpy_pick


@pytest.fixture(scope="module")
def E():
    from openhush_amd import engine
    assert hasattr(engine.lib(), "ohw_lang_pick_host")
    return engine


@pytest.mark.parametrize("preset", ["micro", "micro-v3"])
def test_host_pick_matches_numpy(E, preset):
    hp = synth.PRESETS[preset]
    nl = hp.n_langs
    assert nl == {"micro": 99, "micro-v3": 100}[preset]
    tok = E.SpecialTokens()
    tok.sot, tok.n_langs = SOT, nl
    rows, want = crafted_rows(hp.n_vocab, nl)
    for r, (row, w) in enumerate(zip(rows, want)):
        i, probs = E.lang_pick_host(row, tok)
        ref_i, ref_p = numpy_pick(row, nl)
        top = np.sort(ref_p)[::-1]
        # the rows are not vacuous: the winner (both winners of the tie) stands far above the rest
        assert top[0] - top[2 if r == 2 else 1] > 1e-2
        assert i == w == ref_i, (r, i, w, ref_i)              # np.argmax also returns the first maximum
        assert np.abs(probs - ref_p).max() < 1e-6, (r, float(np.abs(probs - ref_p).max()))
        assert abs(float(probs.astype(np.float64).sum()) - 1.0) < 1e-6
    # the columns outside the range do not move anything: row 3 without its two huge neighbours gives the same result
    plain = rows[3].copy()
    plain[SOT] = plain[SOT + 1 + nl] = 0.0
    i0, p0 = E.lang_pick_host(plain, tok)
    i1, p1 = E.lang_pick_host(rows[3], tok)
    assert i0 == i1 == 33 and np.array_equal(p0, p1)


def test_host_pick_refuses_null(E):
    L = E.lib()
    assert L.ohw_lang_pick_host(None, None, None, None) != 0
