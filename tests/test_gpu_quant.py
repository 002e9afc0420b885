"""Quantised ggml model files (Q4_0, Q4_1, Q5_0, Q5_1, Q8_0) on the GPU: the dequantisation kernel against the library's host twin
bit for bit, contexts loaded from a quantised file against contexts loaded from its f32 twin (same resident weights, same
logits, bit for bit) and against the CPU oracle on the twin (test_gpu_parity.py's tolerances), OHW_DTYPE_AUTO, rejected files,
a mixed file, the pool, the CLI, and large-v3 dims.

Tolerances against the oracle, restated from tests/test_gpu_parity.py (index: 0 bf16, 1 f16):
  encoder  16-bit GEMM operands, fp32 accumulate : bf16 6e-2 / f16 8e-3 abs on O(1) activations (block0 / enc: twice that)
  logits   sigma ~ 4                             : bf16 0.25 / f16 0.03 abs
"""
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

from conftest import ROOT
from openhush_amd import modelfile as M
from openhush_amd import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOL_ACT = {0: 6e-2, 1: 8e-3}
TOL_LOGIT = {0: 0.25, 1: 0.03}
KINDS = ["q4_0", "q4_1", "q5_0", "q5_1", "q8_0"]


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")
    from openhush_amd import engine
    engine.lib()
    return engine


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o
    return o


@pytest.fixture(scope="module")
def qfiles(tmp_path_factory):
    """(preset, kind) -> (quantised file, its f32 twin), written once"""
    d = tmp_path_factory.mktemp("qmodels")
    cache = {}

    def get(preset: str, kind: str, seed: int = 1234):
        key = (preset, kind, seed)
        if key not in cache:
            q = os.path.join(str(d), f"ggml-{preset}-{kind}.bin")
            t = os.path.join(str(d), f"ggml-{preset}-{kind}-f32twin.bin")
            M.write_synthetic_model(q, synth.PRESETS[preset], seed, quant=kind)
            M.write_f32_twin(q, t)
            cache[key] = (q, t)
        return cache[key]

    return get


def random_blocks(kind: str, nb: int, seed: int) -> np.ndarray:
    """random bytes with finite d (and m)"""
    k = M.QUANT_KINDS[kind]
    raw = np.random.default_rng(seed).integers(0, 256, (nb, k.block_bytes), dtype=np.uint8)
    raw[:, 1] &= 0xFB
    if k.has_min:
        raw[:, 3] &= 0xFB
    return raw


def forced_tokens(ctx):
    """the teacher-forced sequence of the committed goldens, written from the context's own special tokens"""
    t = ctx.tok
    return [t.sot, t.sot + 1, t.transcribe, t.timestamp_begin, 48154, 25431, 38077, 28399, 8936, 25727, 47338,
            t.timestamp_begin + 120, t.timestamp_begin + 120, 48859, 48499, 30903, 15765]


def forced_logits(E, ctx, pcm):
    """one window: (mel, taps, logits at positions 3 .. len - 1): a prompt of 4 tokens in one call, then one token per call"""
    st = E.State(ctx, 1)
    mel = st.mel(pcm[None, :], [pcm.size], E.OHW_MEL_REFLECT)
    st.encode(1)
    taps = {k: st.fetch(k, 1)[0] for k in ("conv1", "stem", "block0", "enc")}
    forced = forced_tokens(ctx)
    rows = [st.decode(np.asarray([forced[:4]], np.int32), [0])[0]]
    for i in range(4, len(forced)):
        rows.append(st.decode(np.asarray([[forced[i]]], np.int32), [i])[0])
    return mel[0], taps, np.stack(rows)


@pytest.mark.parametrize("kind", KINDS)
def test_kernel_equals_host_twin_bit_for_bit(E, kind):
    tt = M.QUANT_KINDS[kind].ttype
    for n in (32, 32 * 1000 + 32, 1280 * 5120):
        raw = random_blocks(kind, n // 32, 1000 + n % 977)
        host = E.dequantize_host(tt, raw, n)
        dev = E.dbg_dequantize(tt, raw, n, 0)
        assert np.array_equal(dev.view(np.uint32), host.view(np.uint32)), (kind, n)
    # blocks a quantiser wrote, too
    x = np.random.default_rng(3).standard_normal(32 * 4099).astype(np.float32)
    raw = M.quantize_blocks(x, kind)
    assert np.array_equal(E.dbg_dequantize(tt, raw, x.size, 0).view(np.uint32), M.dequantize_blocks(raw, kind, x.size).view(np.uint32))
    for bad_ttype, bad_n in ((0, 32), (1, 32), (12, 32), (tt, 48), (tt, 0)):
        with pytest.raises(E.WhisperError):
            E.dbg_dequantize(bad_ttype, raw, bad_n, 0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("preset", ["micro", "micro-v3", "tiny"])
def test_quantised_file_equals_its_f32_twin_and_matches_the_oracle(E, oracle, qfiles, preset, kind):
    qpath, tpath = qfiles(preset, kind)
    om = oracle.Model.load(tpath)
    pcm = synth.synth_audio(7)
    ref = None
    for dt in (E.OHW_DTYPE_BF16, E.OHW_DTYPE_F16):
        cq = E.Context.from_file(qpath, 0, dt)
        ct = E.Context.from_file(tpath, 0, dt)
        assert cq.dtype == dt and ct.dtype == dt
        assert cq.hp.ftype == M.QUANT_KINDS[kind].ftype and ct.hp.ftype == 0      # the reduced ftype, not the header word
        dq, dtw = cq.weight_digests(), ct.weight_digests()
        assert len(dq) > 20 and list(dq) == list(dtw)
        assert {k for k in dq if dq[k] != dtw[k]} == set()
        mel, taps, lq = forced_logits(E, cq, pcm)
        _, _, lt = forced_logits(E, ct, pcm)
        assert np.isfinite(lq).all()
        assert np.array_equal(lq.view(np.uint32), lt.view(np.uint32)), (preset, kind, dt)
        del ct
        # the GPU on the quantised file against the CPU oracle on the twin
        if ref is None:
            r_enc, r_c1, r_stem, r_b0 = om.encode(mel, taps=True)
            s = oracle.State(om)
            s.set_encoder_output(om.encode(mel))
            ref = (r_enc, r_c1, r_stem, r_b0, s.decode(forced_tokens(cq), 0, all_pos=True))
        r_enc, r_c1, r_stem, r_b0, r_logits = ref
        tol = TOL_ACT[dt]
        errs = [float(np.abs(taps[k] - r).max()) for k, r in (("conv1", r_c1), ("stem", r_stem), ("block0", r_b0), ("enc", r_enc))]
        worst = max(float(np.abs(lq[i - 3] - r_logits[i]).max()) for i in range(3, len(r_logits)))
        print(f"{preset} {kind} dtype {dt}: conv1 {errs[0]:.2e} stem {errs[1]:.2e} block0 {errs[2]:.2e} enc {errs[3]:.2e} logits {worst:.3e}")
        assert errs[0] < tol and errs[1] < tol and errs[2] < 2 * tol and errs[3] < 2 * tol, errs
        assert worst < TOL_LOGIT[dt], worst
    om.close()


def test_auto_dtype_is_f16_for_a_quantised_file(E, qfiles):
    for kind in KINDS:
        qpath, tpath = qfiles("micro", kind)
        assert E.Context.from_file(qpath, 0, E.OHW_DTYPE_AUTO).dtype == E.OHW_DTYPE_F16, kind
    assert E.Context.from_file(tpath, 0, E.OHW_DTYPE_AUTO).dtype == E.OHW_DTYPE_BF16      # an ftype-0 file: as before


def test_bad_files_are_load_failures(E, qfiles, tmp_path):
    qpath, _ = qfiles("micro", "q5_0")
    hp, filt, vocab, raw = M.read_model_raw(qpath)
    header = hp.as_list()
    assert header[10] == 2008
    victim = next(i for i, t in enumerate(raw) if t.ttype == 6)
    p = str(tmp_path / "ggml-bad.bin")

    def rejected(header_, tensors, *words):
        M.write_model(p, header_, filt, vocab, tensors)
        with pytest.raises(E.LoadFailed) as ei:
            E.Context.from_file(p, 0, E.OHW_DTYPE_F16)
        assert ei.value.code == E.OHW_E_LOAD_FAILED
        assert all(w in str(ei.value) for w in words), str(ei.value)

    # a block row of 48 values
    t = raw[victim]
    bad = list(raw)
    bad[victim] = M.RawTensor(t.name, (t.shape[0], 48), 6, bytes(t.shape[0] * 48 // 32 * 22))
    rejected(header, bad, t.name, "48")
    # quantisation versions other than 2, a k-quant ftype, an unknown ftype
    rejected(header[:10] + [1008], raw, "version 1")
    rejected(header[:10] + [3008], raw, "version 3")
    rejected(header[:10] + [2012], raw, "k-quants are not supported")
    rejected(header[:10] + [2005], raw, "ftype 5")
    # a tensor type the reader does not know (Q4_K)
    bad = list(raw)
    bad[victim] = M.RawTensor(t.name, t.shape, 12, t.data)
    rejected(header, bad, "12")
    # cut in the middle of a block
    cut = list(raw[:victim]) + [M.RawTensor(t.name, t.shape, 6, t.data[:len(t.data) - 11])]
    rejected(header, cut, "truncated")
    # the process is intact: the good file still loads
    M.write_model(p, header, filt, vocab, raw)
    assert E.Context.from_file(p, 0, E.OHW_DTYPE_F16).weight_digests() == E.Context.from_file(qpath, 0, E.OHW_DTYPE_F16).weight_digests()


def test_mixed_file_goes_by_each_tensor_type(E, tmp_models, tmp_path):
    """a stock f16 file (header ftype 1, no quantisation version) in which ONE tensor is Q8_0: a matrix that goes through
    the LayerNorm fold"""
    hp, filt, vocab, raw = M.read_model_raw(tmp_models("micro"))
    assert hp.ftype == 1
    name = "decoder.blocks.1.mlp.0.weight"
    i = next(k for k, t in enumerate(raw) if t.name == name)
    mixed = list(raw)
    mixed[i] = M.RawTensor(name, raw[i].shape, 8, M.quantize_blocks(M.tensor_values(raw[i]), "q8_0").tobytes())
    mpath, tpath = str(tmp_path / "ggml-mixed.bin"), str(tmp_path / "ggml-mixed-twin.bin")
    M.write_model(mpath, hp.as_list(), filt, vocab, mixed)
    M.write_f32_twin(mpath, tpath)
    assert [t.ttype for t in M.read_model_raw(mpath)[3]].count(8) == 1
    cm, ct, cs = (E.Context.from_file(x, 0, E.OHW_DTYPE_F16) for x in (mpath, tpath, tmp_models("micro")))
    assert cm.hp.ftype == 1
    assert E.Context.from_file(mpath, 0, E.OHW_DTYPE_AUTO).dtype == E.OHW_DTYPE_F16
    dm, dt, ds = cm.weight_digests(), ct.weight_digests(), cs.weight_digests()
    assert dm == dt
    changed = {k for k in dm if dm[k] != ds[k]}
    assert 1 <= len(changed) <= 3, changed      # that layer's w1, the bias the fold adds to and the row sums: nothing else moved
    pcm = synth.synth_audio(9)
    _, _, lm = forced_logits(E, cm, pcm)
    _, _, lt = forced_logits(E, ct, pcm)
    assert np.array_equal(lm.view(np.uint32), lt.view(np.uint32))


def test_pool_replicates_a_quantised_file(E, qfiles):
    qpath, _ = qfiles("micro", "q5_0")
    pcm = np.concatenate([synth.synth_audio(70 + w) for w in range(3)] + [synth.synth_audio(75, 90000)])
    eng = E.WhisperEngine.new(qpath, "auto", False, True, 0, E.OHW_DTYPE_F16, 1)
    ref = eng.transcribe(E.AudioBuffer(pcm, 16000))
    ref_tokens = eng.last_tokens()
    eng.close()
    assert len(ref_tokens) > 0
    pool = E.EnginePool(qpath, "auto", False, [0, 0], E.OHW_DTYPE_F16, 1)     # creation compares the replica's digests with device_ids[0]'s
    assert pool.n_devices == 2
    res = pool.transcribe(E.AudioBuffer(pcm, 16000))
    assert res.text == ref.text and pool.last_tokens() == ref_tokens
    pool.close()


def test_cli_transcribes_with_a_quantised_file(E, qfiles, tmp_path):
    qpath, _ = qfiles("tiny", "q5_0")
    pcm = synth.synth_audio(5, 160000)
    wav = str(tmp_path / "ten.wav")
    with wave.open(wav, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes(np.round(pcm * 32767).astype("<i2").tobytes())
    out = subprocess.run([sys.executable, "-m", "openhush_amd.cli", "transcribe", wav, "--model-path", qpath, "--format", "json"],
                         cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    j = json.loads(out.stdout)
    from openhush_amd import cli
    eng = E.WhisperEngine.new(qpath, "auto", False, True, 0, E.OHW_DTYPE_AUTO, 8)     # what the CLI builds by default
    want = eng.transcribe(E.AudioBuffer(cli.load_wav_file(wav), 16000))
    eng.close()
    assert j["text"] == want.text and j["language"] == want.language and j["model"] == "tiny-q5_0"
    assert len(want.text) > 0


def test_large_v3_dims_q5_0(E, tmp_path):
    """large-v3 dims, Q5_0, written on the spot by the numpy quantiser (about 1.1 GB; no twin: it would be 6 GB).  The
    resident-weight digests are taken after the LayerNorm fold and in engine layout, so they are compared only between a
    quantised file and its twin, at the small dims above; here the raw blocks of three tensors go through the kernel."""
    hp = synth.PRESETS["large-v3"]
    qpath = str(tmp_path / "ggml-large-v3-q5_0.bin")
    M.write_synthetic_model(qpath, hp, 1234, quant="q5_0")
    assert 1.0e9 < os.path.getsize(qpath) < 1.2e9
    ctx = E.Context.from_file(qpath, 0, E.OHW_DTYPE_AUTO)
    assert ctx.dtype == E.OHW_DTYPE_F16 and ctx.hp.ftype == 8 and ctx.hp.n_text_layer == 32
    st = E.State(ctx, 1)
    pcm = synth.synth_audio(7)
    st.mel(pcm[None, :], [pcm.size], E.OHW_MEL_REFLECT)
    st.encode(1)
    t = ctx.tok
    prompt = [t.sot, t.sot + 1, t.transcribe, t.no_timestamps]
    lg = st.decode(np.asarray([prompt], np.int32), [0])[0]
    picks = []
    for step in range(16):
        assert np.isfinite(lg).all(), step
        picks.append(int(lg[:t.eot].argmax()))
        lg = st.decode(np.asarray([[picks[-1]]], np.int32), [len(prompt) + step])[0]
    assert np.isfinite(lg).all() and len(picks) == 16
    names = ["decoder.token_embedding.weight", "encoder.blocks.17.mlp.0.weight", "decoder.blocks.30.cross_attn.key.weight"]
    raw = {x.name: x for x in M.read_model_raw(qpath, only=names)[3]}
    for name in names:
        x = raw[name]
        n = int(np.prod(x.shape))
        assert x.ttype == 6 and len(x.data) == n // 32 * 22
        dev = E.dbg_dequantize(6, x.data, n, 0)
        assert np.array_equal(dev.view(np.uint32), M.dequantize_blocks(x.data, "q5_0", n).view(np.uint32)), name
