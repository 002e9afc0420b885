"""What test_gpu_widths.py takes for granted, checked on the fp32 oracle and on paper, no GPU.

  - the absolute logit tolerances of the 2- and 4-layer models (0.25 bf16, 0.03 f16) carry over to every width because the
    oracle's logits have the same spread at every width: per-row standard deviation 4.0
  - the f16 argmax comparison excuses a differing pick only where the oracle's own top-2 margin is below 2 * 0.03: at most a
    fifth of the compared positions may be that thin, at any width, or the comparison would assert little
  - the decoder GEMM shapes the lane test expects are the ones dec_gemm_pick's rule gives, recomputed here from the rule's words
"""
import os

import numpy as np
import pytest

import width_models as W


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o
    o.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    return o


@pytest.fixture(scope="module")
def mel(oracle):
    """window 0's spectrogram: n_mels = 80 at every width, the filterbank does not depend on the model"""
    om = oracle.Model.synth(W.shallow(128), 1234)
    m = om.log_mel(W.windows()[0], W.MEL_ZERO_TAIL)
    om.close()
    return m


def test_special_tokens_are_the_oracles(oracle):
    om = oracle.Model.synth(W.shallow(128), 1234)
    assert (om.tok_eot, om.tok_sot, om.tok_transcribe, om.tok_beg) == (W.EOT, W.SOT, W.TRANSCRIBE, W.TIMESTAMP_BEGIN)
    om.close()
    for d in W.WIDTHS:
        f = W.forced_tokens(d)
        assert len(f) == W.N_FORCED == 48 and f[:4] == [W.SOT, W.SOT + 1, W.TRANSCRIBE, W.TIMESTAMP_BEGIN]
        assert all(0 <= t < W.EOT for t in f[4:]) and len(set(f[4:])) > 40
        assert W.shallow(d) == [51865, 1500, d, d // 64, 2, 448, d, d // 64, 2, 80, 1]
    assert W.WIDTHS == tuple(range(128, W.MAX_WIDTH + 1, 128)) and min(W.TOO_WIDE) == W.MAX_WIDTH + 128


@pytest.mark.parametrize("d", W.WIDTHS)
def test_oracle_logits_have_the_same_spread_and_few_thin_margins(oracle, mel, d):
    om = oracle.Model.synth(W.shallow(d), 1234)
    s = oracle.State(om)
    s.set_encoder_output(om.encode(mel))
    ref = s.decode(W.forced_tokens(d), 0, all_pos=True)
    s.close()
    om.close()
    assert ref.shape == (W.N_FORCED, 51865) and np.isfinite(ref).all()
    sd = ref.astype(np.float64).std(axis=1)
    thin16 = W.thin_margins(ref, 2 * W.TOL_LOGIT[1])
    thin_bf = W.thin_margins(ref, 2 * W.TOL_LOGIT[0])
    n = W.N_FORCED - W.FIRST_FREE
    print(f"width {d}: logit sigma {sd.min():.3f} .. {sd.max():.3f}; margins below 0.06: {len(thin16)} / {n}, below 0.5: {len(thin_bf)} / {n}")
    assert 3.9 <= sd.min() and sd.max() <= 4.1, (d, float(sd.min()), float(sd.max()))
    assert len(thin16) <= 0.2 * n, (d, thin16)          # a seed that fails this is changed in width_models.py; the cap stays


# ---- the decoder GEMM shapes of the lane test -------------------------------------------------------------------------------
# one layer of a 96-window call on 64 CUs, as read off dec_gemm_pick's comment and conditions by hand
STEP = {512: dict(qkv="4x2", o="1x2", xq="1x2", xo="1x2", fc1="4x2", fc2="1x2"),
        1024: dict(qkv="4x6", o="4x2", xq="1x2", xo="4x2", fc1="4x6", fc2="1x6")}
PROMPT = {512: dict(qkv="4x2", o="4x2", xq="1x2", xo="4x2", fc1="4x6", fc2="1x6"),
          1024: dict(qkv="4x6", o="4x2", xq="4x2", xo="4x2", fc1="4x6", fc2="1x6")}


def _by_the_words(gemm, M, d, cus):
    """the rule once more, written apart from width_models.dec_gemm_shape and only for mt > 2 (a lane's calls)"""
    N, K = W.gemm_dims(gemm, d)
    mt, nt = (M + 15) // 16, (N + 15) // 16
    assert mt > 2
    half_m = (mt + 1) // 2
    ln = gemm in ("qkv", "xq", "fc1")
    if not ln and nt * mt <= 2 * cus:
        return "1x1"
    four = (nt + 3) // 4
    if gemm in ("qkv", "fc1") and K <= 1280 and four * half_m > 2 * cus:       # the four-tile grid is over two rounds
        five = gemm == "fc1" and four > cus
        if five and (nt + 4) // 5 >= 32:
            return "5x6"
        if not five and four >= 32:                                                # only while the all-rows grid has 32 workgroups
            return "4x6"
    largest = ((nt + 1) // 2 if ln else nt) * half_m
    if largest > 2 * cus:
        if K <= 1280:
            return "4x2"
        if not ln:
            return "1x6"
    return "2x2" if ln and nt > cus else "1x2"


def test_lane_shapes_follow_the_stated_rule():
    seen = set()
    for d in W.LANE_WIDTHS:
        assert W.lane_shapes(d, 1) == STEP[d], (d, W.lane_shapes(d, 1))
        assert W.lane_shapes(d, 2) == PROMPT[d], (d, W.lane_shapes(d, 2))
        seen |= set(STEP[d].values()) | set(PROMPT[d].values())
    assert seen >= {"4x6", "4x2", "1x6", "1x2"}
    # and the two statements of the rule agree at every accepted width, on a lane and on the whole device
    for d in W.WIDTHS:
        for cus in (32, 64, 256):
            for M in (33, 96, 192):
                for g in W.LANE_GEMMS:
                    assert W.dec_gemm_shape(g, M, d, cus) == _by_the_words(g, M, d, cus), (g, M, d, cus)


def test_the_rule_agrees_with_the_width_768_lines():
    """test_gpu_lane_ln_forms.py's expectations (cu_budget 32, N = 2112 / 2048 / 2528 at several K) are not model shapes; its
    decode half is: width 768, 96 rows on 32 CUs - QKV 4x6 and mlp.0 5x6 in every pass"""
    for M in (96, 192, 33, 66, 95, 190):
        assert W.dec_gemm_shape("qkv", M, 768, 32) == "4x6"
        assert W.dec_gemm_shape("fc1", M, 768, 32) == "5x6"
    # a 16-row batch takes the fused forms in its step and its two-token prompt pass
    for M in (16, 32):
        for g in ("qkv", "fc1"):
            assert W.dec_gemm_shape(g, M, 768, 32) in ("1x1", "2x1", "2x2", "1x2")


def test_small_batches_never_take_a_lane_shape():
    """the whole-path sweep runs two windows: whatever the width, its calls (2, 8 and 16 rows) stay on the fused forms"""
    for d in W.WIDTHS:
        for M in (2, 8, 16):
            for g in W.GEMMS:
                assert W.dec_gemm_shape(g, M, d, 0) in ("1x1", "2x1", "2x2", "1x2"), (g, M, d)


# ---- the needle cases at 8 and 16 heads ------------------------------------------------------------------------------------
def _needle_keys():
    keys = [("cross", n) for n in W.XA_NEEDLES] + [("chunk", n) for n in W.CHUNK_NEEDLES] + [("self", "plain"), ("self", "slots")]
    return [(f, n, H) for f, n in keys for H in W.NEEDLE_HEADS]


@pytest.mark.parametrize("family,name,H", _needle_keys())
def test_needles_at_real_head_counts_decide_their_rows(family, name, H):
    """the construction holds at H = 8 and 16 (the needle keeps its weight), and a kernel that reads head h & 1 - right for
    every H = 2 case of the needle files - is tens of tolerances off here, on the reference itself"""
    import attn_needles as A
    for pattern in A.PATTERNS:
        c, ref, w = W.needle_case(family, name, pattern, H)
        assert c.H == H and ref.shape == (c.R, 64 * H)
        assert (w >= A.MIN_WEIGHT[pattern]).all(), (pattern, float(w.min()))
        assert np.abs(ref).max() <= 1.0                                   # no poison in any reference row
        folded = A.reference(c, head_map=[h & 1 for h in range(H)])
        rows = np.abs(folded - ref).max(axis=1)
        assert (rows > 10 * A.TOL[0]).all(), (pattern, float(rows.min()))
    if family == "cross":
        want = {8: {"m1_t250": "split", "m5_group5_t8": "group5", "m40_t63": "plain", "m40_t250": "split"},
                16: {"m1_t250": "split", "m5_group5_t8": "group5", "m40_t63": "plain", "m40_t250": "plain"}}[H][name]
        assert W.xa_variant(name, H)[0] == want
