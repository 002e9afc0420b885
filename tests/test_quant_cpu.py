"""ggml block quantisation (Q4_0, Q4_1, Q5_0, Q5_1, Q8_0) without a GPU: the numpy restatement in openhush_amd/modelfile.py and the
library's host twin ohw_dequantize_host against hand-built blocks with literal expected values, against each other bit for bit,
the quantisers' round-trip error against bounds that follow from the format, and the model-file writer / reader / f32 twin.

Block layouts (little-endian, d / m IEEE f16, 32 values per block, j = 0 .. 15):
  Q4_0 18 B {d; qs[16]}        y[j] = ((qs[j] & 15) - 8) d       y[j+16] = ((qs[j] >> 4) - 8) d
  Q4_1 20 B {d; m; qs[16]}     y[j] = (qs[j] & 15) d + m         y[j+16] = (qs[j] >> 4) d + m
  Q5_0 22 B {d; qh; qs[16]}    fifth bit of value j / j+16 = qh bit j / j+16;  y = (x - 16) d
  Q5_1 24 B {d; m; qh; qs[16]} y = x d + m
  Q8_0 34 B {d; i8 qs[32]}     y[j] = qs[j] d
"""
import dataclasses
import struct

import numpy as np
import pytest

from openhush_amd import engine as E
from openhush_amd import modelfile as M
from openhush_amd import synth

KINDS = ["q4_0", "q4_1", "q5_0", "q5_1", "q8_0"]


def f16(v: float) -> bytes:
    b = np.float16(v).tobytes()
    assert float(np.frombuffer(b, "<f2")[0]) == v, "the test's scales must be exact in f16"
    return b


def both(kind: str, raw: bytes, n: int = 32):
    """numpy restatement and the library's host twin on the same blocks"""
    a = M.dequantize_blocks(raw, kind, n)
    b = E.dequantize_host(M.QUANT_KINDS[kind].ttype, raw, n)
    assert a.dtype == np.float32 and b.dtype == np.float32 and a.shape == b.shape == (n,)
    return a, b


def check(kind: str, raw: bytes, expected):
    expected = np.asarray(expected, np.float32)
    for got in both(kind, raw, expected.size):
        assert np.array_equal(got, expected), (kind, got, expected)


def test_block_sizes_and_codes():
    assert {k: (v.ttype, v.ftype, v.block_bytes) for k, v in M.QUANT_KINDS.items()} == {
        "q4_0": (2, 2, 18), "q4_1": (3, 3, 20), "q5_0": (6, 8, 22), "q5_1": (7, 9, 24), "q8_0": (8, 7, 34)}


def test_zero_scale_blocks():
    junk = bytes(range(7, 7 + 32))
    check("q4_0", f16(0.0) + junk[:16], np.zeros(32))
    check("q5_0", f16(0.0) + b"\xa5\x5a\xff\x01" + junk[:16], np.zeros(32))
    check("q8_0", f16(0.0) + junk, np.zeros(32))
    check("q4_1", f16(0.0) + f16(1.5) + junk[:16], np.full(32, 1.5))
    check("q5_1", f16(0.0) + f16(-0.75) + b"\xa5\x5a\xff\x01" + junk[:16], np.full(32, -0.75))


def test_q4_extreme_nibbles():
    # qs[j] = 0x0F for even j (low nibble 15, high nibble 0), 0xF0 for odd j (low 0, high 15)
    qs = bytes(0x0F if j % 2 == 0 else 0xF0 for j in range(16))
    low = [3.5 if j % 2 == 0 else -4.0 for j in range(16)]      # (15 - 8) * 0.5, (0 - 8) * 0.5
    high = [-4.0 if j % 2 == 0 else 3.5 for j in range(16)]
    check("q4_0", f16(0.5) + qs, low + high)
    low = [2.75 if j % 2 == 0 else -1.0 for j in range(16)]     # 15 * 0.25 - 1, 0 * 0.25 - 1
    high = [-1.0 if j % 2 == 0 else 2.75 for j in range(16)]
    check("q4_1", f16(0.25) + f16(-1.0) + qs, low + high)
    # a negative scale (what the Q4_0 quantiser writes when the largest value is positive)
    check("q4_0", f16(-2.0) + bytes([0x80] * 16), [16.0] * 16 + [-0.0] * 16)
    # nibble order inside a byte: value j low, value j + 16 high
    check("q4_0", f16(1.0) + bytes([0x21] + [0x88] * 15), [-7.0] + [0.0] * 15 + [-6.0] + [0.0] * 15)


@pytest.mark.parametrize("bit", [0, 15, 16, 31])
def test_q5_high_bits_one_at_a_time(bit):
    qh = struct.pack("<I", 1 << bit)
    exp = np.full(32, -32.0, np.float32)          # (0 - 16) * 2
    exp[bit] = 0.0                                # (16 - 16) * 2: qh bit b is the fifth bit of value b
    check("q5_0", f16(2.0) + qh + bytes(16), exp)
    exp = np.full(32, 1.0, np.float32)            # 0 * 0.5 + 1
    exp[bit] = 9.0                                # 16 * 0.5 + 1
    check("q5_1", f16(0.5) + f16(1.0) + qh + bytes(16), exp)


def test_q5_extreme_codes():
    check("q5_0", f16(2.0) + b"\xff\xff\xff\xff" + b"\xff" * 16, np.full(32, 30.0))          # (31 - 16) * 2
    check("q5_1", f16(0.5) + f16(1.0) + b"\xff\xff\xff\xff" + b"\xff" * 16, np.full(32, 16.5))   # 31 * 0.5 + 1
    # low nibbles 15 with the fifth bit clear, high nibbles 0 with the fifth bit set
    check("q5_0", f16(1.0) + struct.pack("<I", 0xFFFF0000) + b"\x0f" * 16, [-1.0] * 16 + [0.0] * 16)
    check("q5_1", f16(1.0) + f16(0.0) + struct.pack("<I", 0xFFFF0000) + b"\x0f" * 16, [15.0] * 16 + [16.0] * 16)


def test_q8_extreme_codes():
    q = [-128, 127, 0, 1, -1, 64, -64, 100] + list(range(-12, 12))
    raw = f16(0.125) + np.asarray(q, np.int8).tobytes()
    check("q8_0", raw, [v * 0.125 for v in q])
    check("q8_0", f16(-3.0) + np.asarray([-128, 127] * 16, np.int8).tobytes(), [384.0, -381.0] * 16)


def test_two_blocks_are_independent():
    raw = f16(1.0) + bytes([0x98] * 16) + f16(0.5) + bytes([0x00] * 16)
    check("q4_0", raw, [0.0] * 16 + [1.0] * 16 + [-4.0] * 32)


def test_host_twin_rejects_bad_arguments():
    raw = bytes(34)
    out = np.zeros(64, np.float32)
    L = E.lib()
    import ctypes as C
    src = C.c_char_p(raw)
    for ttype, n in ((0, 32), (1, 32), (4, 32), (12, 32), (8, 0), (8, 31), (8, -32)):
        assert L.ohw_dequantize_host(ttype, src, n, out.ctypes.data_as(C.POINTER(C.c_float))) == E.OHW_E_INVALID_ARG, (ttype, n)
    assert L.ohw_dequantize_host(8, None, 32, out.ctypes.data_as(C.POINTER(C.c_float))) == E.OHW_E_INVALID_ARG
    assert L.ohw_dequantize_host(8, src, 32, None) == E.OHW_E_INVALID_ARG
    with pytest.raises(ValueError):
        M.dequantize_blocks(raw, "q8_0", 48)


def random_blocks(kind: str, nb: int, seed: int) -> np.ndarray:
    """random bytes, the f16 exponents of d (and m) kept below all-ones so that both are finite"""
    k = M.QUANT_KINDS[kind]
    raw = np.random.default_rng(seed).integers(0, 256, (nb, k.block_bytes), dtype=np.uint8)
    raw[:, 1] &= 0xFB
    if k.has_min:
        raw[:, 3] &= 0xFB
    return raw


@pytest.mark.parametrize("kind", KINDS)
def test_host_twin_equals_numpy_bit_for_bit(kind):
    nb = 8192
    raw = random_blocks(kind, nb, 99)
    a, b = both(kind, raw.tobytes(), nb * 32)
    assert np.isfinite(a).all()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # subnormal and tiny scales too
    raw[:, 1] &= 0x83
    a, b = both(kind, raw.tobytes(), nb * 32)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# e = max |dq(q(x)) - x| over a block, d (and m) the fp32 scale before it is stored as f16.  One quantisation step (half a step
# where the quantiser rounds to nearest over the whole range; a whole step for Q4_0 / Q5_0, whose value at -max maps to code
# 16 / 32 and is capped at 15 / 31) plus the f16 rounding of d (relative 2^-11) times the largest code, plus that of m.
def bound(kind: str, d: np.ndarray, m) -> np.ndarray:
    d = np.abs(d.astype(np.float64))
    u = 2.0 ** -11
    if kind == "q8_0":
        return d * (0.5 + 127 * u)
    if kind == "q4_0":
        return d * (1 + 8 * u)
    if kind == "q5_0":
        return d * (1 + 16 * u)
    codes = 15 if kind == "q4_1" else 31
    return d * (0.5 + codes * u) + np.abs(m.astype(np.float64)) * u


@pytest.mark.parametrize("kind", KINDS)
def test_round_trip_error_stays_inside_the_format_bound(kind):
    x = np.random.default_rng(2024).standard_normal((20000, 32)).astype(np.float32)
    raw, d, m = M.quantize_blocks(x, kind, return_scale=True)
    assert raw.shape == (20000, M.QUANT_KINDS[kind].block_bytes) and raw.dtype == np.uint8
    assert np.array_equal(raw, M.quantize_blocks(x, kind))
    y = E.dequantize_host(M.QUANT_KINDS[kind].ttype, raw, x.size).reshape(x.shape)
    e = np.abs(y.astype(np.float64) - x.astype(np.float64)).max(axis=1)
    b = bound(kind, d, m)
    worst = float((e / np.abs(d.astype(np.float64))).max())
    print(f"{kind}: worst e/|d| = {worst:.4f}, worst e/bound = {float((e / b).max()):.4f}")
    assert (e <= b).all(), (kind, worst)


def test_quantisers_on_constant_and_zero_blocks():
    for kind in KINDS:
        z = M.dequantize_blocks(M.quantize_blocks(np.zeros(64, np.float32), kind), kind, 64)
        assert np.array_equal(z, np.zeros(64, np.float32)), kind          # d == 0: 1 / d is taken as 0
    for kind in ("q4_1", "q5_1"):
        c = M.dequantize_blocks(M.quantize_blocks(np.full(32, 0.75, np.float32), kind), kind, 32)
        assert np.array_equal(c, np.full(32, 0.75, np.float32)), kind     # d == 0, m carries the value
    # Q8_0 rounds halves away from zero; with amax = 127 the scale is 1 and the codes are round(x)
    x = np.zeros(32, np.float32)
    x[:6] = [127.0, 0.5, -0.5, 1.5, -2.5, 0.49]
    q = M.quantize_blocks(x, "q8_0")[0, 2:8].view(np.int8)
    assert list(q) == [127, 1, -1, 2, -3, 0]


@pytest.mark.parametrize("kind", KINDS)
def test_written_file_reads_back_and_has_an_f32_twin(kind, tmp_path):
    hp = synth.PRESETS["nano"]
    qpath, tpath = str(tmp_path / f"ggml-nano-{kind}.bin"), str(tmp_path / "ggml-nano-twin.bin")
    M.write_synthetic_model(qpath, hp, 77, quant=kind)
    M.write_f32_twin(qpath, tpath)
    k = M.QUANT_KINDS[kind]
    qhp, qfilt, qvocab, qraw = M.read_model_raw(qpath)
    assert qhp.ftype == k.ftype + 2000
    assert qhp.as_list()[:10] == hp.as_list()[:10]
    specs = synth.tensor_specs(hp)
    assert [t.name for t in qraw] == [s.name for s in specs]
    src = dataclasses.replace(hp, ftype=1)      # the values an ftype-1 file of this seed stores are what gets quantised
    _, _, _, values = M.read_model(qpath)
    n_quant = 0
    for spec, t in zip(specs, qraw):
        stored = synth.gen_tensor(77, spec, src)
        if len(spec.shape) == 2 and spec.name.endswith(".weight"):
            n_quant += 1
            assert t.ttype == k.ttype, spec.name
            blocks = M.quantize_blocks(stored, kind)
            assert t.data == blocks.tobytes(), spec.name
            want = M.dequantize_blocks(blocks, kind, stored.size).reshape(spec.shape)
        else:
            assert t.ttype == (1 if spec.f16 else 0), spec.name
            want = stored
        assert np.array_equal(values[spec.name].view(np.uint32), want.view(np.uint32)), spec.name
    assert n_quant == 1 + 6 * hp.n_audio_layer + 10 * hp.n_text_layer
    thp, tfilt, tvocab, traw = M.read_model_raw(tpath)
    assert thp.ftype == 0 and thp.as_list()[:10] == hp.as_list()[:10]
    assert np.array_equal(tfilt, qfilt) and tvocab == qvocab
    assert [(t.name, t.shape) for t in traw] == [(t.name, t.shape) for t in qraw]
    assert all(t.ttype == 0 for t in traw)
    for t in traw:
        assert np.array_equal(M.tensor_values(t).view(np.uint32), values[t.name].view(np.uint32)), t.name


def test_stock_writer_is_unchanged_by_the_quant_argument(tmp_path):
    hp = synth.PRESETS["nano"]
    a, b = str(tmp_path / "a.bin"), str(tmp_path / "b.bin")
    M.write_synthetic_model(a, hp, 5)
    M.write_synthetic_model(b, hp, 5, quant=None)
    assert open(a, "rb").read() == open(b, "rb").read()
    hp2, _, _, raw = M.read_model_raw(a)
    assert hp2.ftype == 1 and {t.ttype for t in raw} == {0, 1}


def test_reader_rejects_a_block_row_that_is_not_a_multiple_of_32(tmp_path):
    p = str(tmp_path / "bad.bin")
    hp = synth.PRESETS["nano"]
    M.write_model(p, hp.as_list()[:10] + [2008], synth.mel_filterbank(hp.n_mels), [b"a"],
                  [M.RawTensor("x.weight", (2, 48), 6, bytes(3 * 22))])
    with pytest.raises(ValueError):
        M.read_model_raw(p)
