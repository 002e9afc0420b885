"""stitch_kernel (ohw_dbg_stitch / ohw_stitch_seams) on the shared table of tests/stitch_ref.py: every int32 word of every seam
equals the Python restatement, poison behind n_text is never read, the guard seams behind the output keep their sentinel, and
one window launches nothing."""
import numpy as np
import pytest

import stitch_ref as S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from openhush_amd import engine
    assert hasattr(engine.lib(), "ohw_dbg_stitch")
    return engine


def _report(got, want, names):
    bad = np.flatnonzero((got != want).any(axis=1))
    return [(int(s), names[s // 2] if s % 2 == 0 else "between", got[s].tolist(), want[s].tolist()) for s in bad[:5]]


def test_every_word_of_the_table_equals_the_restatement_and_the_guards_hold(E):
    tok, n_text, names, want = S.table()
    assert tok.shape == (300, S.STRIDE)
    got = E.dbg_stitch((tok, n_text), n_guard=5, sentinel=S.SENTINEL)
    assert got.shape == (304, 8)
    assert _report(got[:299], want, names) == []
    assert (got[299:] == S.SENTINEL).all()
    # the entry the engine calls, and the host twin on the same table
    assert (E.stitch_seams((tok, n_text)) == want).all() and (E.stitch_seams_host((tok, n_text)) == want).all()


def test_a_narrow_table_and_two_windows(E):
    """a stride that is no multiple of anything, the sides full: the right row starts at an odd word of LDS"""
    rng = np.random.default_rng(8)
    tok = rng.integers(0, 5, (7, 37)).astype(np.int32)
    n_text = np.array([37, 37, 0, 36, 1, 37, 2], np.int32)
    want = S.seams(tok, n_text)
    got = E.dbg_stitch((tok, n_text), n_guard=2, sentinel=S.SENTINEL)
    assert (got[:6] == want).all(), (got[:6].tolist(), want.tolist())
    assert (got[6:] == S.SENTINEL).all()
    a, b = list(range(100, 140)), list(range(130, 180))
    assert E.stitch_seams([a, b]).tolist() == S.seams([a, b], None).tolist() == [[0, 10, 10, 35, 5, 40, 50, 0]]


def test_one_window_launches_nothing(E):
    tok, n_text, _, _ = S.table()
    got = E.dbg_stitch((tok[:1], n_text[:1]), n_guard=3, sentinel=S.SENTINEL)
    assert got.shape == (3, 8) and (got == S.SENTINEL).all()
    assert E.stitch_seams((tok[:1], n_text[:1])).shape == (0, 8)
    with pytest.raises(E.WhisperError):
        E.dbg_stitch((tok[:2], np.array([3, 449], np.int32)))                  # a count past the stride is refused, not clamped
