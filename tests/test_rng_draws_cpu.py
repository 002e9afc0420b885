"""The draws of the device temperature ladder: the host keeps whisper.cpp's std::mt19937 generators and hands the device
their draws in advance (ohw_rng_uniforms), then advances each generator by the draws a pass kept (ohw_rng_discard_draws).
A draw of std::discrete_distribution is one std::generate_canonical<double, 53> (two engine outputs, low word first) and
the pick is the lower bound of it in the normalised partial sums - the oracle restates both (whisper_ref.c mt_canonical,
discrete_draw).  No GPU: the generator entries need no context, the probabilities come from the oracle's filter."""
import ctypes as C
import os

import numpy as np
import pytest

from openhush_amd import engine as E, synth
from oracle import oracle

from conftest import GOLDEN


def _mt_canonical(r: "oracle.MT19937") -> float:
    """whisper_ref.c mt_canonical: std::generate_canonical<double, 53> over a 32-bit engine as libstdc++ evaluates it"""
    s = float(r.next())
    s += float(r.next()) * 4294967296.0
    x = s / 18446744073709551616.0
    return x if x < 1.0 else float(np.nextafter(1.0, 0.0))


def test_uniforms_are_the_canonical_doubles_bit_for_bit():
    rng, ref = E.HostRng(0), oracle.MT19937(0)
    u = rng.uniforms(1000)
    want = np.array([_mt_canonical(ref) for _ in range(1000)], np.float64)
    assert u.tobytes() == want.tobytes()
    assert rng.uniforms(1000).tobytes() == u.tobytes()            # drawn from a copy: the generator did not move
    assert np.all((u >= 0.0) & (u < 1.0)) and len(np.unique(u)) == 1000
    assert rng.uniforms(0).size == 0


def test_discard_draws_advances_by_whole_draws():
    for n in (0, 1, 7, 311, 312, 313, 1000):          # 312 draws = 624 outputs: one twist of the state
        rng, ref = E.HostRng(0), oracle.MT19937(0)
        rng.discard_draws(n)
        for _ in range(n):
            _mt_canonical(ref)
        want = np.array([_mt_canonical(ref) for _ in range(3)], np.float64)
        assert rng.uniforms(3).tobytes() == want.tobytes(), n
    # in steps: the same place as in one call
    a, b = E.HostRng(0), E.HostRng(0)
    for k in (3, 0, 50, 1):
        a.discard_draws(k)
    b.discard_draws(54)
    assert a.uniforms(5).tobytes() == b.uniforms(5).tobytes()
    with pytest.raises(E.WhisperError):
        E._check(E.lib().ohw_rng_discard_draws(a.h, -1))


@pytest.fixture(scope="module")
def rows():
    g = np.load(os.path.join(GOLDEN, "sampler.npz"))
    r = g["rows_f16"].astype(np.float32)
    hists = [[int(t) for t in g["hists"][g["hist_of_row"][i]] if t >= 0] for i in range(r.shape[0])]
    return r, hists


def _filtered_probs(om, op, row, hist, T):
    """the oracle's filter at temperature T -> (probabilities as float32 expf(logprob), 0 where masked) - what
    ohw_sample_host hands std::discrete_distribution"""
    L = oracle.lib()
    lg = np.ascontiguousarray(row, np.float32).copy()
    lps = np.zeros_like(lg)
    cur = np.asarray(hist or [0], np.int32)
    lp, ns = C.c_float(0), C.c_float(0)
    fp = C.POINTER(C.c_float)
    L.ref_process_logits_ex(om.h, C.byref(op), lg.ctypes.data_as(fp), cur.ctypes.data_as(C.POINTER(C.c_int32)), len(hist), C.cast(None, fp), T,
                            lps.ctypes.data_as(fp), C.byref(lp), C.byref(ns))
    p = np.where(lg == -np.inf, np.float32(0), np.exp(lps.astype(np.float32)))
    return p.astype(np.float32)


def _lower_bound(p: np.ndarray, u: float) -> int:
    """std::discrete_distribution's pick: normalised double partial sums (last = 1), first index with cp >= u"""
    pd = p.astype(np.float64)
    cp = np.cumsum(pd / pd.sum())
    cp[-1] = 1.0
    return int(np.searchsorted(cp, u, side="left"))


def test_predrawn_path_matches_a_shared_generator_draw_for_draw(rows):
    """On the sampler goldens' rows, with and without history, at T = 0.2, 0.6 and 1.0: the pre-drawn path (ohw_rng_uniforms
    of one HostRng, the lower bound in host code, ohw_rng_discard_draws(1) per step) picks what the oracle's sampler picks
    drawing step by step from one shared MT19937(0) (ref_sample_step: its own canonical draw and cumulative search over the
    same filtered row).  A different pick is allowed only where the draw lies within 1e-9 of an interval edge."""
    r, hists = rows
    hp = synth.PRESETS["nano"]
    om = oracle.Model.synth(hp.as_list(), 1234)
    op = om.default_params()
    L = oracle.lib()
    fp = C.POINTER(C.c_float)
    L.ref_sample_step.argtypes = [C.c_void_p, C.POINTER(oracle.SampleParams), fp, C.POINTER(C.c_int32), C.c_int, fp, C.c_float,
                                  C.POINTER(oracle.MT19937), fp, fp, C.POINTER(C.c_double), fp]
    rng, orng = E.HostRng(0), oracle.MT19937(0)
    picks, n, n_hist_rows = set(), 0, 0
    for T in (0.2, 0.6, 1.0):
        for i in range(r.shape[0]):
            for hist in ([], hists[i]) if hists[i] else ([],):
                n_hist_rows += bool(hist)
                u = rng.uniforms(1)[0]
                mine = _lower_bound(_filtered_probs(om, op, r[i], hist, T), u)
                rng.discard_draws(1)
                lg = r[i].copy()
                cur = np.asarray(hist or [0], np.int32)
                olp, gap = C.c_float(0), C.c_double(0)
                theirs = L.ref_sample_step(om.h, C.byref(op), lg.ctypes.data_as(fp), cur.ctypes.data_as(C.POINTER(C.c_int32)), len(hist), None, T,
                                           C.byref(orng), C.byref(olp), None, C.byref(gap), None)
                assert mine == theirs or gap.value < 1e-9, (T, i, len(hist), mine, theirs, gap.value)
                picks.add(mine)
                n += 1
    assert n_hist_rows > 0 and n > 40
    assert len(picks) > 10                      # the draws really vary
    # both sides consumed one draw per step: the generators still agree
    assert rng.uniforms(1)[0] == _mt_canonical(orng)
