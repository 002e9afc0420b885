"""Shapes and token paths of the width sweep (test_widths_cpu.py, test_gpu_widths.py).  Host arithmetic only: no GPU, no library.

A model's width picks template instantiations and launch shapes (LayerNorm's MAXV, the decoder GEMM's work shape, the encoder
GEMM's kernel, the head count of every attention launch), so every width the loader accepts gets a model of its own: two encoder
and two decoder layers - every per-layer kernel and the layer-to-layer hand-off; depth is test_gpu_decoder_depth.py's subject.
"""
import numpy as np

# every width the loader accepts: multiples of 128 up to the fused LayerNorm's widest K (kernels.hpp, DG_LN_MAXK), d_head 64
WIDTHS = (128, 256, 384, 512, 640, 768, 896, 1024, 1152, 1280)
MAX_WIDTH = 1280
TOO_WIDE = (1408, 2048, 2176)      # the first width past the limit, launch_layernorm's widest d, the first past that one

TOL_ACT = {0: 6e-2, 1: 8e-3}       # test_gpu_parity.py: bf16, f16
TOL_LOGIT = {0: 0.25, 1: 0.03}
N_FORCED = 48
FIRST_FREE = 3                     # positions 0 .. 2 are inside the prompt pass: position 3 is the first whose row is a pick

# the multilingual vocabulary's special ids at n_vocab = 51865 (model.hip, set_special_tokens; checked against the oracle's table
# in test_widths_cpu.py)
EOT, SOT, TRANSCRIBE, TIMESTAMP_BEGIN = 50257, 50258, 50359, 50364


def shallow(d, n_mels=80, n_vocab=51865, n_layer=2):
    """hparams list of a width-d model with n_layer encoder and n_layer decoder layers"""
    return [n_vocab, 1500, d, d // 64, n_layer, 448, d, d // 64, n_layer, n_mels, 1]


def forced_tokens(d):
    """[sot, language, transcribe, timestamp_begin], then 44 text ids drawn for this width: 48 positions"""
    rng = np.random.default_rng(d)
    return [SOT, SOT + 1, TRANSCRIBE, TIMESTAMP_BEGIN] + [int(t) for t in rng.integers(0, EOT, N_FORCED - 4)]


def thin_margins(ref, thr):
    """positions FIRST_FREE .. of the reference logits [n][V] whose top-2 margin is below thr"""
    out = []
    for i in range(FIRST_FREE, len(ref)):
        top = np.partition(ref[i], -2)[-2:]
        if float(top[1] - top[0]) < thr:
            out.append(i)
    return out


# ---- the decoder GEMM's work shape ------------------------------------------------------------------------------------------
# dec_gemm_pick's rule (decode.hip) in its own words, for the default path (LayerNorm prologue, no split-K), with
# mt = ceil(M / 16), nt = ceil(N / 16), cus = the stream's CU budget:
#   out-projections and mlp.2 (residual epilogue): one tile per workgroup while mt == 1 or nt * mt <= 2 cus
#   LN forms with mt <= 2: 1x1 while nt * mt <= cus, else 2x1 while ceil(nt / 2) * mt <= cus or mt == 1
#   logits with mt == 1: 2x1
#   LN1 + QKV and LN2 + mlp.0, mt > 2, K <= 1280, ceil(nt / 4) * ceil(mt / 2) > 2 cus (the four-tile grid is over two rounds):
#       the all-rows forms - mlp.0 with ceil(nt / 4) > cus: 5x6 if ceil(nt / 5) >= 32; otherwise 4x6 if ceil(nt / 4) >= 32
#   every form but mlp.2's K: mt > 2, K <= 1280 and the largest grid so far (LN: ceil(nt / 2) * ceil(mt / 2), else
#       nt * ceil(mt / 2)) > 2 cus: 4x2
#   residual epilogue, mt > 2, K > 1280, nt * ceil(mt / 2) > 2 cus: 1x6
#   LN with nt > cus, and logits: 2x2; everything else 1x2
GEMMS = ("qkv", "o", "xq", "xo", "fc1", "fc2", "logits")
LN_GEMMS = ("qkv", "xq", "fc1")


def _cdiv(a, b):
    return -(-a // b)


def gemm_dims(gemm, d, n_vocab=51865):
    """(N, K) of a decoder GEMM at width d"""
    return {"qkv": (3 * d, d), "o": (d, d), "xq": (d, d), "xo": (d, d), "fc1": (4 * d, d), "fc2": (d, 4 * d), "logits": (n_vocab, d)}[gemm]


def dec_gemm_shape(gemm, M, d, cus, n_vocab=51865):
    """the work shape ("4x6" ...) the rule above gives a decoder GEMM of M rows at width d on a stream of `cus` CUs (0: all 256)"""
    N, K = gemm_dims(gemm, d, n_vocab)
    cus = cus if cus > 0 else 256
    mt, nt = _cdiv(M, 16), _cdiv(N, 16)
    ln, resid = gemm in LN_GEMMS, gemm in ("o", "xo", "fc2")
    if resid and (mt == 1 or nt * mt <= 2 * cus):
        return "1x1"
    if ln and mt <= 2:
        if nt * mt <= cus:
            return "1x1"
        if _cdiv(nt, 2) * mt <= cus or mt == 1:
            return "2x1"
    if gemm == "logits" and mt == 1:
        return "2x1"
    if gemm in ("qkv", "fc1") and mt > 2 and K <= MAX_WIDTH and _cdiv(nt, 4) * _cdiv(mt, 2) > 2 * cus:
        if gemm == "fc1" and _cdiv(nt, 4) > cus:
            if _cdiv(nt, 5) >= 32:
                return "5x6"
        elif _cdiv(nt, 4) >= 32:
            return "4x6"
    grid = (_cdiv(nt, 2) if ln else nt) * _cdiv(mt, 2)
    if mt > 2 and K <= MAX_WIDTH and grid > 2 * cus:
        return "4x2"
    if resid and mt > 2 and K > MAX_WIDTH and nt * _cdiv(mt, 2) > 2 * cus:
        return "1x6"
    if (ln and nt > cus) or gemm == "logits":
        return "2x2"
    return "1x2"


def counter_name(gemm, shape):
    """ohw_dbg_counter's name of a (GEMM, shape) tally on the default path"""
    return f"dec_gemm.{gemm}{'.ln' if gemm in LN_GEMMS else ''}.{shape}"


SHAPES = ("1x1", "2x1", "1x2", "2x2", "4x2", "1x6", "4x6", "5x6")


def tally_names():
    """every decoder-variant counter name (include/ohw.h, ohw_dbg_counter)"""
    names = [f"dec_gemm.{g}{f}.{s}" for g in GEMMS for f in ("", ".ln", ".pn", ".ks") for s in SHAPES]
    names += ["xattn." + v for v in ("plain", "split", "rows2", "rows3", "rows4", "group2", "group3", "group4", "group5", "group_split", "chunk")]
    names += ["self_attn." + v for v in ("plain", "slots", "fused", "fused_slots")]
    return names


# the lane of test_gpu_widths.py (c): 96 windows on a 64-CU stream; a two-token prompt pass (192 rows), then single-token steps
LANE_ROWS = 96
LANE_CUS = 64
LANE_WIDTHS = (512, 1024)
LANE_GEMMS = ("qkv", "o", "xq", "xo", "fc1", "fc2")


def lane_shapes(d, n_new):
    """{gemm: shape} of one layer of a LANE_ROWS-window call of n_new tokens per window on the lane"""
    return {g: dec_gemm_shape(g, LANE_ROWS * n_new, d, LANE_CUS) for g in LANE_GEMMS}


# ---- the two windows of the whole-path sweep --------------------------------------------------------------------------------
WINDOW_SAMPLES = (480000, 48000)   # one full window, one 3 s recording (zero tail)
MEL_ZERO_TAIL = 1                  # OHW_MEL_ZERO_TAIL (include/ohw.h), the oracle's log_mel mode 1


def windows():
    """pcm [2][480000] of the sweep: window 1 holds 3 s of signal and zeros behind it"""
    from openhush_amd import synth
    pcm = np.zeros((2, synth.CHUNK_SAMPLES), np.float32)
    pcm[0] = synth.synth_audio(7)
    pcm[1, :WINDOW_SAMPLES[1]] = synth.synth_audio(3, WINDOW_SAMPLES[1])
    return pcm


# ---- attention needles at the product's head counts (tests/attn_needles.py; every case there runs H = 2) ---------------------
NEEDLE_HEADS = (8, 16)             # base and medium
# name -> (M, t_len, kv_group, invariant): single-token rows; the variant launch_cross_attn picks follows from xattn_split at H
XA_NEEDLES = {"m1_t250": (1, 250, 1, False), "m5_group5_t8": (5, 8, 5, True), "m40_t63": (40, 63, 1, False), "m40_t250": (40, 250, 1, False)}
CHUNK_NEEDLES = {8: (3, 33), 16: (2, 33)}      # n_q -> (windows, t_len): a ragged second 32-key block
_needles = {}


def xa_variant(name, H):
    import attn_needles as A
    M, t_len, kv_group, _ = XA_NEEDLES[name]
    if kv_group > 1:
        return f"group{kv_group}", 1
    ks = A.xattn_split(M, H, t_len)
    return ("split" if ks > 1 else "plain"), ks


def needle_case(family, name, pattern, H):
    """(case, float64 reference [R][64 H], needle weights [R][H]) built once and shared; treat as read-only.
    family "cross": XA_NEEDLES; "chunk": name = n_q; "self": name = "plain" | "slots", attn_needles.N_PAST, one new token"""
    import attn_needles as A
    key = (family, name, pattern, H)
    if key not in _needles:
        seed = [ord(ch) for ch in f"width{family}{name}{pattern}"] + [H]
        if family == "cross":
            M, t_len, kv_group, _ = XA_NEEDLES[name]
            c = A.cross_case(seed, pattern, M, 1, t_len, kv_group, ks=xa_variant(name, H)[1], H=H)
        elif family == "chunk":
            n_win, t_len = CHUNK_NEEDLES[name]
            c = A.cross_case(seed, pattern, name * n_win, name, t_len, H=H)
        else:
            c = A.self_case(seed, pattern, A.N_PAST, 1, A.N_CTX, slots=name == "slots", H=H)
        ref, w = A.reference(c, weights=True)
        for a in (c.q, c.K, c.V, ref, w):
            a.setflags(write=False)
        _needles[key] = (c, ref, w)
    return _needles[key]
