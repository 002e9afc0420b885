"""ggml `ggml-*.bin` Whisper model files: writer (synthetic models) and reader (checks).

Format as described in SURVEY.md Appendix A (the only format the reference downloads:
reference src/engine/whisper.rs:71-102).  Layout:
  u32 magic 0x67676d6c
  11 x i32 hparams  (n_vocab, n_audio_ctx, n_audio_state, n_audio_head, n_audio_layer,
                     n_text_ctx, n_text_state, n_text_head, n_text_layer, n_mels, ftype)
  i32 n_mel, i32 n_fft(=201), n_mel*n_fft f32 mel filters
  i32 n_tokens, then n_tokens x { u32 len, bytes }
  tensors until EOF: { i32 n_dims, i32 name_len, i32 ttype (0 f32, 1 f16, 2 Q4_0, 3 Q4_1, 6 Q5_0, 7 Q5_1, 8 Q8_0),
                       i32 dims[n_dims] (fastest-varying first), name bytes, raw data }
Quantised files: the header's ftype word is ftype + 1000 * quantisation version (2); ftype 2 / 3 / 7 / 8 / 9 = mostly
Q4_0 / Q4_1 / Q8_0 / Q5_0 / Q5_1.  Only the 2-D `*.weight` tensors are quantised, in blocks of 32 values along the fastest
dimension (QUANT_KINDS, quantize_blocks, dequantize_blocks); everything else stays f16 / f32.
Parity of this reader/writer with real files is unpinned (no real file exists offline): the block layouts and the
quantisers restate the published format.
"""
from __future__ import annotations

import dataclasses
import mmap
import os
import struct
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import synth

GGML_MAGIC = 0x67676D6C


def synthetic_vocab(hp: synth.HParams) -> List[bytes]:
    """A stand-in vocabulary: printable byte strings for text tokens.  The stock files carry
    only the text tokens (< eot) plus nothing for specials; whisper.cpp synthesises names for the
    rest.  We write n_vocab - (specials) entries exactly like the stock converter (eot index)."""
    n_text = 50257 if hp.is_multilingual else 50256
    words = []
    for i in range(n_text):
        words.append((" w%d" % i).encode("ascii"))
    words[220] = b" "   # the real multilingual vocabulary has " " at 220 (suppress_blank target)
    return words


# ---------------------------------------------------------------------------------------------
# block quantisation: 32 values per block, d / m stored as IEEE f16, little-endian
#   q4_0 18 B {d; u8 qs[16]}          q4_1 20 B {d; m; u8 qs[16]}
#   q5_0 22 B {d; u32 qh; u8 qs[16]}  q5_1 24 B {d; m; u32 qh; u8 qs[16]}      q8_0 34 B {d; i8 qs[32]}
# value j of a block sits in the low nibble of qs[j] (j < 16) or the high nibble of qs[j - 16]; its fifth bit is qh bit j
# ---------------------------------------------------------------------------------------------
QK = 32


class QuantKind(NamedTuple):
    ttype: int         # per-tensor type code
    ftype: int         # header code of a file that is "mostly" this kind
    block_bytes: int
    bits: int          # 4, 5 or 8
    has_min: bool      # q4_1 / q5_1: y = q * d + m


QUANT_KINDS: Dict[str, QuantKind] = {
    "q4_0": QuantKind(2, 2, 18, 4, False),
    "q4_1": QuantKind(3, 3, 20, 4, True),
    "q5_0": QuantKind(6, 8, 22, 5, False),
    "q5_1": QuantKind(7, 9, 24, 5, True),
    "q8_0": QuantKind(8, 7, 34, 8, False),
}
QUANT_BY_TTYPE = {k.ttype: name for name, k in QUANT_KINDS.items()}
QUANT_VERSION = 2


def _inv(d: np.ndarray) -> np.ndarray:
    """1 / d in fp32, 0 where d == 0"""
    with np.errstate(divide="ignore"):
        return np.where(d != 0, np.float32(1.0) / d, np.float32(0.0)).astype(np.float32)


def quantize_blocks(x: np.ndarray, kind: str, return_scale: bool = False):
    """ggml's reference quantisers, restated: x (size a multiple of 32, rows of 32 along the fastest dimension) -> uint8
    [n / 32][block_bytes].  With return_scale: also the fp32 d (and m, or None) of every block BEFORE their rounding to f16."""
    k = QUANT_KINDS[kind]
    x = np.ascontiguousarray(x, np.float32).reshape(-1, QK)
    nb = x.shape[0]
    rows = np.arange(nb)
    m = None
    if kind == "q8_0":
        d = (np.abs(x).max(axis=1) / np.float32(127.0)).astype(np.float32)
        v = (x * _inv(d)[:, None]).astype(np.float64)
        q = (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int8)      # roundf: halves away from zero
    elif not k.has_min:
        # max: the value of largest magnitude (the first such), with its sign; it maps to code 0, -max past the last code
        top = np.float32(1 << (k.bits - 1))
        mx = x[rows, np.abs(x).argmax(axis=1)]
        d = (mx / -top).astype(np.float32)
        v = (x * _inv(d)[:, None]).astype(np.float32) + (top + np.float32(0.5))
        q = np.minimum(v.astype(np.int8), (1 << k.bits) - 1).astype(np.uint8)
    else:
        m = x.min(axis=1)
        d = ((x.max(axis=1) - m) / np.float32((1 << k.bits) - 1)).astype(np.float32)
        v = ((x - m[:, None]) * _inv(d)[:, None]).astype(np.float32) + np.float32(0.5)
        q = np.minimum(v.astype(np.uint8), (1 << k.bits) - 1).astype(np.uint8)
    out = np.empty((nb, k.block_bytes), np.uint8)
    out[:, 0:2] = d.astype("<f2").view(np.uint8).reshape(nb, 2)
    off = 2
    if k.has_min:
        out[:, 2:4] = m.astype("<f2").view(np.uint8).reshape(nb, 2)
        off = 4
    if kind == "q8_0":
        out[:, off:] = q.view(np.uint8)
    else:
        if k.bits == 5:
            bit = ((q >> 4) & 1).astype(np.uint32)
            qh = (bit << np.arange(QK, dtype=np.uint32)[None, :]).sum(axis=1, dtype=np.uint32)
            out[:, off:off + 4] = qh.astype("<u4").view(np.uint8).reshape(nb, 4)
            off += 4
        out[:, off:] = (q[:, :16] & 15) | ((q[:, 16:] & 15) << 4)
    if return_scale:
        return out, d, m
    return out


def dequantize_blocks(raw, kind: str, n: int) -> np.ndarray:
    """n / 32 blocks (bytes or uint8 array) -> float32 [n]: fp32 after widening d and m, multiply then add (two roundings)"""
    k = QUANT_KINDS[kind]
    if n % QK != 0:
        raise ValueError("n must be a multiple of 32")
    nb = n // QK
    b = np.frombuffer(raw, np.uint8) if isinstance(raw, (bytes, bytearray, memoryview)) else np.ascontiguousarray(raw, np.uint8).reshape(-1)
    if b.size < nb * k.block_bytes:
        raise ValueError("block data is truncated")
    b = b[:nb * k.block_bytes].reshape(nb, k.block_bytes)
    d = np.ascontiguousarray(b[:, 0:2]).view("<f2").astype(np.float32)          # [nb][1]
    off = 2
    m = None
    if k.has_min:
        m = np.ascontiguousarray(b[:, 2:4]).view("<f2").astype(np.float32)
        off = 4
    if kind == "q8_0":
        y = np.ascontiguousarray(b[:, off:]).view(np.int8).astype(np.float32) * d
        return y.reshape(-1)
    hi = np.zeros((nb, QK), np.int32)
    if k.bits == 5:
        qh = np.ascontiguousarray(b[:, off:off + 4]).view("<u4").astype(np.uint32)   # [nb][1]
        j = np.arange(16, dtype=np.uint32)[None, :]
        hi[:, :16] = ((qh >> j) << np.uint32(4)) & np.uint32(16)
        hi[:, 16:] = (qh >> (j + np.uint32(12))) & np.uint32(16)
        off += 4
    qs = b[:, off:].astype(np.int32)
    q = np.concatenate([qs & 15, qs >> 4], axis=1) | hi
    if k.has_min:
        y = (q.astype(np.float32) * d).astype(np.float32) + m
    else:
        y = (q - (1 << (k.bits - 1))).astype(np.float32) * d
    return y.astype(np.float32).reshape(-1)


def is_quantised_tensor(spec: synth.TensorSpec) -> bool:
    """what whisper.cpp's quantiser converts: the 2-D `*.weight` tensors; conv weights, biases, LayerNorms and positional
    embeddings stay f16 / f32"""
    return len(spec.shape) == 2 and spec.name.endswith(".weight")


def write_synthetic_model(path: str, hp: synth.HParams, seed: int = 1234, quant: Optional[str] = None) -> None:
    """quant = None: hp.ftype as given (0 all f32, 1 the stock f16 layout).  quant = "q4_0" | "q4_1" | "q5_0" | "q5_1" | "q8_0":
    the header carries ftype = code + 2000 and the 2-D `*.weight` tensors are quantised (from the values an ftype-1 file of
    the same seed stores); the rest is written as in an ftype-1 file."""
    header = hp.as_list()
    if quant is not None:
        hp = dataclasses.replace(hp, ftype=1)
        header = hp.as_list()
        header[10] = QUANT_KINDS[quant].ftype + 1000 * QUANT_VERSION
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        f.write(struct.pack("<I", GGML_MAGIC))
        f.write(struct.pack("<11i", *header))
        filt = synth.mel_filterbank(hp.n_mels)
        f.write(struct.pack("<2i", hp.n_mels, synth.N_FREQ))
        f.write(filt.astype("<f4").tobytes())
        vocab = synthetic_vocab(hp)
        f.write(struct.pack("<i", len(vocab)))
        for w in vocab:
            f.write(struct.pack("<I", len(w)))
            f.write(w)
        # the generator is element-wise numpy (the GIL is released inside it): tensors are made by a few threads, a
        # bounded number ahead of the writer, and written in the file's order (large-v3 = 3.1 GB: 90 s -> 15 s)
        import concurrent.futures as cf
        specs = synth.tensor_specs(hp)

        def make(spec):
            if quant is not None and is_quantised_tensor(spec):
                return quantize_blocks(synth.gen_tensor(seed, spec, hp), quant), QUANT_KINDS[quant].ttype
            as_f16 = spec.f16 and hp.ftype == 1
            return synth.gen_tensor(seed, spec, hp).astype("<f2" if as_f16 else "<f4"), 1 if as_f16 else 0

        workers = max(1, min(8, len(os.sched_getaffinity(0))))
        with cf.ThreadPoolExecutor(max_workers=workers) as ex:
            pending = []
            it = iter(specs)
            for spec in it:
                pending.append((spec, ex.submit(make, spec)))
                if len(pending) < 2 * workers:
                    continue
                _write_tensor(f, *pending.pop(0))
            while pending:
                _write_tensor(f, *pending.pop(0))
    os.replace(tmp, path)


def _write_tensor(f, spec, fut) -> None:
    arr, ttype = fut.result()
    name = spec.name.encode("ascii")
    dims = list(reversed(spec.shape))
    f.write(struct.pack("<3i", len(dims), len(name), ttype))
    f.write(struct.pack("<%di" % len(dims), *dims))
    f.write(name)
    f.write(arr.tobytes() if arr.size < (1 << 20) else memoryview(arr).cast("B"))


class RawTensor(NamedTuple):
    name: str
    shape: Tuple[int, ...]   # row-major (numpy order)
    ttype: int
    data: bytes              # as stored in the file


def tensor_bytes(ttype: int, n: int) -> int:
    if ttype in QUANT_BY_TTYPE:
        return n // QK * QUANT_KINDS[QUANT_BY_TTYPE[ttype]].block_bytes
    if ttype not in (0, 1):
        raise ValueError("unsupported tensor type %d" % ttype)
    return n * (2 if ttype == 1 else 4)


def read_model_raw(path: str, only: Optional[Sequence[str]] = None) -> Tuple[synth.HParams, np.ndarray, List[bytes], List[RawTensor]]:
    """the file as it is: hparams (ftype: the header word, quantisation version included), mel filters, vocabulary and every
    tensor's stored bytes, in file order.  only: names whose bytes are wanted (the others come back with empty data) - a
    gigabyte file is then mapped, not read."""
    with open(path, "rb") as f:
        buf = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) if only is not None else f.read()
    off = 0
    (magic,) = struct.unpack_from("<I", buf, off); off += 4
    if magic != GGML_MAGIC:
        raise ValueError("bad magic 0x%08x" % magic)
    vals = struct.unpack_from("<11i", buf, off); off += 44
    hp = synth.HParams(*vals)
    n_mel, n_fft = struct.unpack_from("<2i", buf, off); off += 8
    filt = np.frombuffer(buf, "<f4", n_mel * n_fft, off).reshape(n_mel, n_fft).copy(); off += 4 * n_mel * n_fft
    (n_tok,) = struct.unpack_from("<i", buf, off); off += 4
    vocab = []
    for _ in range(n_tok):
        (ln,) = struct.unpack_from("<I", buf, off); off += 4
        vocab.append(bytes(buf[off:off + ln])); off += ln
    tensors: List[RawTensor] = []
    while off < len(buf):
        n_dims, name_len, ttype = struct.unpack_from("<3i", buf, off); off += 12
        dims = struct.unpack_from("<%di" % n_dims, buf, off); off += 4 * n_dims
        name = bytes(buf[off:off + name_len]).decode("ascii"); off += name_len
        shape = tuple(reversed(dims))
        if ttype in QUANT_BY_TTYPE and dims[0] % QK != 0:
            raise ValueError("quantised tensor %s: first dimension %d is not a multiple of 32" % (name, dims[0]))
        nbytes = tensor_bytes(ttype, int(np.prod(shape)))
        if off + nbytes > len(buf):
            raise ValueError("model file is truncated")
        keep = only is None or name in only
        tensors.append(RawTensor(name, shape, ttype, bytes(buf[off:off + nbytes]) if keep else b"")); off += nbytes
    return hp, filt, vocab, tensors


def tensor_values(t: RawTensor) -> np.ndarray:
    """float32 array of a stored tensor, quantised ones expanded by dequantize_blocks"""
    n = int(np.prod(t.shape))
    if t.ttype in QUANT_BY_TTYPE:
        return dequantize_blocks(t.data, QUANT_BY_TTYPE[t.ttype], n).reshape(t.shape)
    return np.frombuffer(t.data, "<f2" if t.ttype == 1 else "<f4", n).reshape(t.shape).astype(np.float32)


def read_model(path: str) -> Tuple[synth.HParams, np.ndarray, List[bytes], Dict[str, np.ndarray]]:
    hp, filt, vocab, raw = read_model_raw(path)
    return hp, filt, vocab, {t.name: tensor_values(t) for t in raw}


def write_model(path: str, header: Sequence[int], filt: np.ndarray, vocab: List[bytes], tensors: Sequence[RawTensor]) -> None:
    """any file of this format from its parts (header: the 11 hparams words as they go into the file)"""
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        f.write(struct.pack("<I", GGML_MAGIC))
        f.write(struct.pack("<11i", *[int(v) for v in header]))
        f.write(struct.pack("<2i", *filt.shape))
        f.write(np.ascontiguousarray(filt, "<f4").tobytes())
        f.write(struct.pack("<i", len(vocab)))
        for w in vocab:
            f.write(struct.pack("<I", len(w)))
            f.write(w)
        for t in tensors:
            name = t.name.encode("ascii")
            dims = list(reversed(t.shape))
            f.write(struct.pack("<3i", len(dims), len(name), t.ttype))
            f.write(struct.pack("<%di" % len(dims), *dims))
            f.write(name)
            f.write(t.data)
    os.replace(tmp, path)


def write_f32_twin(src_path: str, twin_path: str) -> None:
    """the f32 twin of a (quantised) file: the same tensors in the same order, ftype = 0, every tensor stored as ttype 0 -
    the quantised ones holding dequantize_blocks(...) of their blocks.  What a reader that knows only f32 / f16 (the CPU
    oracle) loads to compute with exactly the weights the quantised file expands to."""
    hp, filt, vocab, raw = read_model_raw(src_path)
    header = hp.as_list()
    header[10] = 0
    twins = [RawTensor(t.name, t.shape, 0, tensor_values(t).astype("<f4").tobytes()) for t in raw]
    write_model(twin_path, header, filt, vocab, twins)
