"""The legacy 32-weight ggml block formats (Q4_0, Q4_1, Q5_0, Q5_1) without a GPU: the NumPy
reference against a literal scalar decoder, the quantiser's error, the GGUF writer / reader,
the planar repack and the C++ CPU backend."""
import struct

import numpy as np
import pytest

from llama_fastapi_k8s_gpu_amd.engine.llama import Llama
from llama_fastapi_k8s_gpu_amd.gguf.constants import GGML_BLOCK, GGMLType, tensor_nbytes
from llama_fastapi_k8s_gpu_amd.gguf.quants import dequantize, quantize
from llama_fastapi_k8s_gpu_amd.gguf.reader import GGUFReader
from llama_fastapi_k8s_gpu_amd.gguf.synthetic import (SPECS, build_vocab, tensor_plan, write_synthetic_gguf)
from llama_fastapi_k8s_gpu_amd.models.llama import ReferenceLlama
from llama_fastapi_k8s_gpu_amd.runtime import load_cpu

NEW = [GGMLType.Q4_0, GGMLType.Q4_1, GGMLType.Q5_0, GGMLType.Q5_1]
BYTES = {GGMLType.Q4_0: 18, GGMLType.Q4_1: 20, GGMLType.Q5_0: 22, GGMLType.Q5_1: 24}
HAS_M = (GGMLType.Q4_1, GGMLType.Q5_1)
HAS_H = (GGMLType.Q5_0, GGMLType.Q5_1)


def _f16(b):
    return np.float32(np.frombuffer(bytes(b), dtype="<f2")[0])


def scalar_fields(t, blk):
    """One block's fields straight from the format table: d, m (f32 values of the f16 fields)
    and the 32 unsigned quants, weight by weight (independent of quants.py)."""
    blk = bytes(blk)
    o = 0
    d = _f16(blk[o:o + 2]); o += 2
    m = np.float32(0)
    if t in HAS_M:
        m = _f16(blk[o:o + 2]); o += 2
    qh = 0
    if t in HAS_H:
        qh = struct.unpack("<I", blk[o:o + 4])[0]; o += 4
    qs = blk[o:o + 16]
    q = [0] * 32
    for j in range(16):
        lo, hi = qs[j] & 0xF, qs[j] >> 4
        if t in HAS_H:
            lo |= ((qh >> j) & 1) << 4
            hi |= ((qh >> (j + 16)) & 1) << 4
        q[j], q[j + 16] = lo, hi
    return d, m, q


def scalar_decode_block(t, blk):
    d, m, q = scalar_fields(t, blk)
    out = np.empty(32, np.float32)
    for j in range(32):
        if t == GGMLType.Q4_0:
            out[j] = d * np.float32(q[j] - 8)
        elif t == GGMLType.Q5_0:
            out[j] = d * np.float32(q[j] - 16)
        else:
            out[j] = d * np.float32(q[j]) + m
    return out


def _random_blocks_finite(t, nb, rng):
    raw = np.frombuffer(rng.bytes(nb * BYTES[t]), np.uint8).reshape(nb, BYTES[t]).copy()
    d = rng.uniform(-2.0, 2.0, nb).astype(np.float16)
    raw[:, 0:2] = d.reshape(-1, 1).view(np.uint8)
    if t in HAS_M:
        raw[:, 2:4] = rng.uniform(-3.0, 3.0, nb).astype(np.float16).reshape(-1, 1).view(np.uint8)
    return raw


# ---------------------------------------------------------------- 1. format exactness
@pytest.mark.parametrize("t", NEW)
def test_block_sizes(t):
    assert GGML_BLOCK[t] == (32, BYTES[t])
    assert tensor_nbytes(t, 32 * 7) == 7 * BYTES[t]


@pytest.mark.parametrize("t", NEW)
def test_dequantize_equals_scalar_decoder(t):
    rng = np.random.default_rng(100 + int(t))
    raw = _random_blocks_finite(t, 64, rng)
    got = dequantize(raw.reshape(-1), t, 64 * 32).reshape(64, 32)
    want = np.stack([scalar_decode_block(t, raw[i]) for i in range(64)])
    assert got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("t", [GGMLType.Q5_0, GGMLType.Q5_1])
@pytest.mark.parametrize("qh,hot", [(0x00010001, (0, 16)), (0x80008000, (15, 31))])
def test_fifth_bit_positions(t, qh, hot):
    """All-zero qs: only the weights whose qh bit is set carry the 5th bit (value 16)."""
    d, m = np.float16(0.5), np.float16(-1.25)
    blk = d.tobytes() + (m.tobytes() if t in HAS_M else b"") + struct.pack("<I", qh) + bytes(16)
    assert len(blk) == BYTES[t]
    got = dequantize(np.frombuffer(blk, np.uint8), t, 32)
    q = np.zeros(32, np.float32)
    q[list(hot)] = 16
    want = np.float32(0.5) * (q - 16) if t == GGMLType.Q5_0 else np.float32(0.5) * q + np.float32(-1.25)
    assert np.array_equal(got, want.astype(np.float32))
    assert np.array_equal(got, scalar_decode_block(t, blk))


def test_q4_one_block_by_hand():
    qs = bytes((j | ((15 - j) << 4)) for j in range(16))   # weight j = j, weight 16 + j = 15 - j
    d = np.float16(2.0)
    got0 = dequantize(np.frombuffer(d.tobytes() + qs, np.uint8), GGMLType.Q4_0, 32)
    q = np.concatenate([np.arange(16), 15 - np.arange(16)]).astype(np.float32)
    assert np.array_equal(got0, 2.0 * (q - 8))
    m = np.float16(-3.0)
    got1 = dequantize(np.frombuffer(d.tobytes() + m.tobytes() + qs, np.uint8), GGMLType.Q4_1, 32)
    assert np.array_equal(got1, 2.0 * q - 3.0)


@pytest.mark.parametrize("t", NEW)
def test_f16_arithmetic_is_one_rounding(t):
    """arith="f16": every weight is ONE f16 rounding of q * a + b with the stored f16 pair
    (a, b) = (d, -8d) / (d, -16d) / (d, m)."""
    rng = np.random.default_rng(7 + int(t))
    raw = _random_blocks_finite(t, 64, rng)
    got = dequantize(raw.reshape(-1), t, 64 * 32, arith="f16").reshape(64, 32)
    for i in range(64):
        d, m, q = scalar_fields(t, raw[i])
        a = np.float64(d)
        b = np.float64(m) if t in HAS_M else np.float64(np.float16(-(8 if t == GGMLType.Q4_0 else 16) * a))
        want = (np.asarray(q, np.float64) * a + b).astype(np.float16).astype(np.float32)
        assert np.array_equal(got[i], want), i


# ---------------------------------------------------------------- 2. round trip
# relative RMS error of quantize -> dequantize on 2^16 N(0, 1) samples, measured with seed 0:
#   Q4_0 0.0862   Q4_1 0.0782   Q5_0 0.0428   Q5_1 0.0380
# (Q4_K measures 0.078 and Q5_K 0.038 with the same data); the bounds are 1.5 x those values
MEASURED = {GGMLType.Q4_0: 0.0862, GGMLType.Q4_1: 0.0782, GGMLType.Q5_0: 0.0428, GGMLType.Q5_1: 0.0380}


@pytest.mark.parametrize("t", NEW)
@pytest.mark.parametrize("seed", [0, 1])
def test_quantize_roundtrip_error(t, seed):
    x = np.random.default_rng(seed).standard_normal(1 << 16).astype(np.float32)
    raw = quantize(x, t)
    assert raw.size == tensor_nbytes(t, x.size)
    y = dequantize(raw, t, x.size)
    rel = float(np.sqrt(np.mean((y - x) ** 2)) / np.sqrt(np.mean(x ** 2)))
    assert rel < 1.5 * MEASURED[t], rel


# ---------------------------------------------------------------- 3. writer / reader
def test_legacy_mixed_gguf_roundtrip(tmp_path):
    spec = SPECS["tiny-llama3-legacy-mixed"]
    path = write_synthetic_gguf(spec, str(tmp_path / "m.gguf"), seed=1)
    rd = GGUFReader(path)
    _, n_vocab = build_vocab(spec)
    plan = tensor_plan(spec, n_vocab)
    seen = set()
    for name, t, shape in plan:
        ti = rd.tensors[name]
        assert GGMLType(ti.ggml_type) == t, name
        n = int(np.prod(shape))
        assert ti.n_elements == n
        assert np.asarray(rd.raw(name)).nbytes == tensor_nbytes(t, n), name
        seen.add(t)
    assert set(NEW) | {GGMLType.Q8_0} <= seen


@pytest.mark.parametrize("name,t,ftype", [("tiny-llama3-q4_0", GGMLType.Q4_0, 2), ("tiny-llama3-q5_1", GGMLType.Q5_1, 9),
                                          ("tiny-q5_0-oddff", GGMLType.Q5_0, 8), ("llama3-8b-q4_0", GGMLType.Q4_0, 2)])
def test_uniform_legacy_plans(name, t, ftype):
    from llama_fastapi_k8s_gpu_amd.gguf.synthetic import hparams_metadata
    spec = SPECS[name]
    plan = tensor_plan(spec, 512)
    for tname, tt, shape in plan:
        if len(shape) < 2:
            assert tt == GGMLType.F32
        elif tname == "output.weight":
            assert tt == GGMLType.Q6_K
        else:
            assert tt == t, tname
    assert hparams_metadata(spec, 512)["general.file_type"] == ftype


# ---------------------------------------------------------------- 4. planar repack
def _planar_numpy(t, raw, R, K):
    """The layout of csrc/common.h: qs[R][K/32][16] | (qh[R][K/32] u32) | d or (d, m) [R][K/32]."""
    nb = K // 32
    b = raw.reshape(R, nb, BYTES[t])
    o = 4 if t in HAS_M else 2
    sc = b[:, :, 0:o]
    planes = []
    if t in HAS_H:
        qh = b[:, :, o:o + 4]
        o += 4
    qs = b[:, :, o:o + 16]
    planes.append(qs.reshape(-1))
    if t in HAS_H:
        planes.append(qh.reshape(-1))
    planes.append(sc.reshape(-1))
    return np.concatenate(planes)


def _repack():
    return load_cpu().repack


@pytest.mark.parametrize("t", NEW)
def test_repack_planar_layout(t):
    rng = np.random.default_rng(int(t))
    R, K = 70, 576
    raw = np.frombuffer(rng.bytes(R * (K // 32) * BYTES[t]), np.uint8).copy()
    full = _repack()(int(t), raw, K, 0, R, 0, K, R, 0, 0)
    assert full.size == raw.size   # the planar copy keeps the GGUF byte count
    assert np.array_equal(full, _planar_numpy(t, raw, R, K))
    # a row slice with r0 > 0
    r0, Rs = 13, 40
    rows = raw.reshape(R, -1)[r0:r0 + Rs].reshape(-1)
    part = _repack()(int(t), raw, K, r0, Rs, 0, K, Rs, 0, 0)
    assert np.array_equal(part, _planar_numpy(t, rows, Rs, K))
    # a column slice (whole blocks)
    c0, Kd = 64, 256
    cols = raw.reshape(R, K // 32, BYTES[t])[:, c0 // 32:(c0 + Kd) // 32].reshape(-1)
    part = _repack()(int(t), raw, K, 0, R, c0, Kd, R, 0, 0)
    assert np.array_equal(part, _planar_numpy(t, cols, R, Kd))


@pytest.mark.parametrize("t", NEW)
def test_repack_gate_up_interleave(t):
    rng = np.random.default_rng(50 + int(t))
    F, K = 64, 256
    nbytes = (K // 32) * BYTES[t]
    g = np.frombuffer(rng.bytes(F * nbytes), np.uint8).copy()
    u = np.frombuffer(rng.bytes(F * nbytes), np.uint8).copy()
    planar = _repack()(int(t), g, K, 0, F, 0, K, 2 * F, 32, 0) | _repack()(int(t), u, K, 0, F, 0, K, 2 * F, 32, 32)
    # destination rows: 32 gate rows, then the 32 up rows of the same features, and so on
    rows = np.empty((2 * F, nbytes), np.uint8)
    for f in range(F):
        rows[(f // 32) * 64 + f % 32] = g.reshape(F, nbytes)[f]
        rows[(f // 32) * 64 + 32 + f % 32] = u.reshape(F, nbytes)[f]
    assert np.array_equal(planar, _planar_numpy(t, rows.reshape(-1), 2 * F, K))


# ---------------------------------------------------------------- 5. CPU backend
CPU_MODELS = ["tiny-llama3-q4_0", "tiny-llama3-q5_1", "tiny-llama3-legacy-mixed"]


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    d = tmp_path_factory.mktemp("legacy_models")
    return {m: write_synthetic_gguf(m, str(d / f"{m}.gguf")) for m in CPU_MODELS}


def _rel(a, b):
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-12))


@pytest.mark.parametrize("model", CPU_MODELS)
def test_cpu_prefill_logits_match_reference(paths, model):
    """As tests/test_cpu_backend.py::test_prefill_logits_match_reference, with its bound (0.06)."""
    cpu = load_cpu()
    path = paths[model]
    ref = ReferenceLlama(GGUFReader(path), n_ctx=64)
    toks = [int(t) for t in np.random.default_rng(1).integers(3, 500, 20)]
    want = ref.forward(toks, 0).numpy()
    eng = cpu.CpuEngine(path, n_ctx=64, n_threads=4, n_batch=8)
    got = eng.eval_logits(toks, 0)
    assert got.shape == want.shape
    assert _rel(got, want) < 0.06, _rel(got, want)
    want2 = ref.forward([7], len(toks)).numpy()
    assert _rel(eng.eval_logits([7], len(toks)), want2) < 0.06


@pytest.mark.parametrize("model", CPU_MODELS)
def test_cpu_greedy_generation_matches_reference_backend(paths, model):
    path = paths[model]
    a = Llama(path, n_ctx=96, backend="cpu", seed=0, n_threads=4)
    b = Llama(path, n_ctx=96, backend="reference", seed=0)
    ra = a.create_completion("the quick brown fox", max_tokens=8, temperature=0.0)
    rb = b.create_completion("the quick brown fox", max_tokens=8, temperature=0.0)
    ta = a.tokenize(ra["choices"][0]["text"].encode(), add_bos=False)
    tb = b.tokenize(rb["choices"][0]["text"].encode(), add_bos=False)
    # the near-tie rule of tests/test_cpu_backend.py: q8 activations can flip a near-tie late
    n = 0
    while n < min(len(ta), len(tb)) and ta[n] == tb[n]:
        n += 1
    assert n >= min(3, len(tb))


def test_cpu_engine_clean_under_asan_ubsan(paths):
    """The stand-alone ASan + UBSan driver (repack, CPU engine) over a model that holds all four
    formats: no report, and it generates (as tests/test_sanitizers.py does for the other types)."""
    import os
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("needs g++ with libasan/libubsan")
    from llama_fastapi_k8s_gpu_amd.runtime.build import build_sanitize_driver
    try:
        driver = build_sanitize_driver()
    except RuntimeError as e:  # toolchain without the sanitizer runtimes
        pytest.skip(f"sanitizer build unavailable: {e}")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = subprocess.run([driver, "run", paths["tiny-llama3-legacy-mixed"], "6"], capture_output=True, text=True,
                       env=env, timeout=120)
    assert "AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, r.stdout + r.stderr
    assert "generated=6" in r.stdout


# ---------------------------------------------------------------- 6. MoE experts are refused
def test_legacy_expert_tensors_are_refused(tmp_path):
    from dataclasses import replace
    spec = replace(SPECS["tiny-mixtral-q4_k_m"], name="tiny-mixtral-q4_0", quant="q4_0")
    path = write_synthetic_gguf(spec, str(tmp_path / "moe.gguf"))
    with pytest.raises(RuntimeError, match=r"ffn_(gate|up|down)_exps\.weight.*Q4_0"):
        load_cpu().CpuEngine(path, n_ctx=64, n_threads=2, n_batch=8)
