"""The 2- and 3-bit K-quants (Q2_K, Q3_K) without a GPU: the NumPy reference against blocks built
by hand from the format's formulas, the quantiser's error, the synthetic mixes through the GGUF
writer and both readers, the planar repack and the C++ CPU backend."""
from dataclasses import replace

import numpy as np
import pytest

from llama_fastapi_k8s_gpu_amd.gguf.constants import GGML_BLOCK, GGMLType, tensor_nbytes
from llama_fastapi_k8s_gpu_amd.gguf.quants import dequantize, quantize, random_blocks
from llama_fastapi_k8s_gpu_amd.gguf.reader import GGUFReader
from llama_fastapi_k8s_gpu_amd.gguf.synthetic import (SPECS, build_vocab, hparams_metadata, tensor_plan,
                                                     tensor_types, write_synthetic_gguf)
from llama_fastapi_k8s_gpu_amd.models.llama import ReferenceLlama
from llama_fastapi_k8s_gpu_amd.runtime import load_cpu

Q2_K, Q3_K = GGMLType.Q2_K, GGMLType.Q3_K
NEW = [Q2_K, Q3_K]
BYTES = {Q2_K: 84, Q3_K: 110}


def _f16(b):
    return np.float32(np.frombuffer(bytes(b), dtype="<f2")[0])


def formula_q2k(blk):
    """The 256 weights of one Q2_K block, weight by weight from the format's formulas."""
    blk = bytes(blk)
    scales, qs = blk[0:16], blk[16:80]
    d, dmin = _f16(blk[80:82]), _f16(blk[82:84])
    out = np.empty(256, np.float32)
    for i in range(256):
        n, j, l, s = i // 128, (i % 128) // 32, i % 32, i // 16
        q = (qs[32 * n + l] >> (2 * j)) & 3
        out[i] = d * np.float32(scales[s] & 0xF) * np.float32(q) - dmin * np.float32(scales[s] >> 4)
    return out


def q3k_fields(blk):
    """(q in -4..3 [256], sc - 32 [16], d) of one Q3_K block from the format's formulas."""
    blk = bytes(blk)
    hmask, qs, scales = blk[0:32], blk[32:96], blk[96:108]
    d = _f16(blk[108:110])
    sc = []
    for s in range(16):
        low = (scales[s] & 0xF) if s < 8 else (scales[s - 8] >> 4)
        top = (scales[8 + s % 4] >> (2 * (s // 4))) & 3
        sc.append((low | (top << 4)) - 32)
    q = []
    for i in range(256):
        n, j, l = i // 128, (i % 128) // 32, i % 32
        q.append(((qs[32 * n + l] >> (2 * j)) & 3) + 4 * ((hmask[l] >> (4 * n + j)) & 1) - 4)
    return q, sc, d


def formula_q3k(blk):
    q, sc, d = q3k_fields(blk)
    return np.array([d * np.float32(sc[i // 16]) * np.float32(q[i]) for i in range(256)], np.float32)


FORMULA = {Q2_K: formula_q2k, Q3_K: formula_q3k}


def _random_blocks_finite(t, nb, rng):
    raw = np.frombuffer(rng.bytes(nb * BYTES[t]), np.uint8).reshape(nb, BYTES[t]).copy()
    d = rng.uniform(-2.0, 2.0, nb).astype(np.float16).reshape(-1, 1).view(np.uint8)
    if t == Q2_K:
        raw[:, 80:82] = d
        raw[:, 82:84] = rng.uniform(-3.0, 3.0, nb).astype(np.float16).reshape(-1, 1).view(np.uint8)
    else:
        raw[:, 108:110] = d
    return raw


# ---------------------------------------------------------------- 1. format exactness
@pytest.mark.parametrize("t", NEW)
def test_block_sizes(t):
    assert GGML_BLOCK[t] == (256, BYTES[t])
    assert tensor_nbytes(t, 256 * 7) == 7 * BYTES[t]


def test_q2k_one_block_by_hand():
    scales = bytes(((3 * s + 1) & 0xF) | (((5 * s + 2) & 0xF) << 4) for s in range(16))
    qs = bytes((37 * b + 11) & 0xFF for b in range(64))
    blk = scales + qs + np.float16(0.75).tobytes() + np.float16(0.375).tobytes()
    assert len(blk) == 84
    got = dequantize(np.frombuffer(blk, np.uint8), Q2_K, 256)
    want = formula_q2k(blk)
    assert got.dtype == np.float32
    assert np.array_equal(got, want)
    # spot values written out: weight 0 (n 0, j 0, l 0, s 0) and weight 255 (n 1, j 3, l 31, s 15)
    assert got[0] == np.float32(0.75 * 1 * (11 & 3) - 0.375 * 2)
    q255 = (qs[63] >> 6) & 3
    assert got[255] == np.float32(0.75 * ((3 * 15 + 1) & 0xF) * q255 - 0.375 * ((5 * 15 + 2) & 0xF))


def test_q3k_one_block_by_hand():
    """A set and an unset hmask bit in both 128-halves, and a scale from each of the four 6-bit
    packing groups (s = 1, 5, 9, 13)."""
    hmask = bytearray(32)
    qs = bytes((29 * b + 7) & 0xFF for b in range(64))
    # weights (n, j, l): set bits for (0, 1, 3) and (1, 2, 5); (0, 1, 4) and (1, 2, 6) stay unset
    hmask[3] |= 1 << (4 * 0 + 1)
    hmask[5] |= 1 << (4 * 1 + 2)
    want_sc = {1: 45, 5: 7, 9: 63, 13: 18}   # 6-bit values: sub-blocks 1, 5 (low nibbles), 9, 13 (high)
    scales = bytearray(12)
    for s, v in want_sc.items():
        if s < 8:
            scales[s] |= v & 0xF
        else:
            scales[s - 8] |= (v & 0xF) << 4
        scales[8 + s % 4] |= (v >> 4) << (2 * (s // 4))
    blk = bytes(hmask) + qs + bytes(scales) + np.float16(-0.5).tobytes()
    assert len(blk) == 110
    got = dequantize(np.frombuffer(blk, np.uint8), Q3_K, 256)
    assert np.array_equal(got, formula_q3k(blk))
    q, sc, d = q3k_fields(blk)
    for s, v in want_sc.items():
        assert sc[s] == v - 32
    i_set0, i_unset0 = 0 * 128 + 1 * 32 + 3, 0 * 128 + 1 * 32 + 4      # sub-block 2 (scale 0 - 32)
    i_set1, i_unset1 = 1 * 128 + 2 * 32 + 5, 1 * 128 + 2 * 32 + 6      # sub-block 12
    for i, l, n, j, hb in ((i_set0, 3, 0, 1, 1), (i_unset0, 4, 0, 1, 0), (i_set1, 5, 1, 2, 1), (i_unset1, 6, 1, 2, 0)):
        qi = ((qs[32 * n + l] >> (2 * j)) & 3) + 4 * hb - 4
        assert q[i] == qi
        assert got[i] == np.float32(-0.5) * np.float32(sc[i // 16]) * np.float32(qi)
    # the weights of sub-blocks 1, 5, 9, 13 use the packed scales
    for s, v in want_sc.items():
        i = 16 * s + 2
        assert got[i] == np.float32(-0.5) * np.float32(v - 32) * np.float32(q[i])


@pytest.mark.parametrize("t", NEW)
def test_dequantize_equals_formula(t):
    rng = np.random.default_rng(100 + int(t))
    raw = _random_blocks_finite(t, 24, rng)
    got = dequantize(raw.reshape(-1), t, 24 * 256).reshape(24, 256)
    want = np.stack([FORMULA[t](raw[i]) for i in range(24)])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("t", NEW)
def test_f16_arithmetic_is_one_rounding(t):
    """arith="f16": the sub-block scale is f16(d * sc) (and f16(-dmin * m) for Q2_K), each from an
    f32 product, and every weight is ONE f16 rounding of q * a + b."""
    rng = np.random.default_rng(7 + int(t))
    raw = _random_blocks_finite(t, 24, rng)
    got = dequantize(raw.reshape(-1), t, 24 * 256, arith="f16").reshape(24, 256)
    f32 = dequantize(raw.reshape(-1), t, 24 * 256).reshape(24, 256)
    for i in range(24):
        blk = bytes(raw[i])
        if t == Q2_K:
            d, dmin = _f16(blk[80:82]), _f16(blk[82:84])
            a = [np.float64(np.float16(d * np.float32(blk[s] & 0xF))) for s in range(16)]
            b = [np.float64(np.float16(-dmin * np.float32(blk[s] >> 4))) for s in range(16)]
            q = [(blk[16 + 32 * (k // 128) + k % 32] >> (2 * ((k % 128) // 32))) & 3 for k in range(256)]
        else:
            q, sc, d = q3k_fields(blk)
            a = [np.float64(np.float16(d * np.float32(sc[s]))) for s in range(16)]
            b = [np.float64(0)] * 16
        want = np.array([np.float64(q[k]) * a[k // 16] + b[k // 16] for k in range(256)]).astype(np.float16)
        assert np.array_equal(got[i], want.astype(np.float32)), i
    # f16 rounding only: the scale, the offset and the result each round once (2^-11 relative);
    # |q| <= 4 scales the first, so |diff| <= 2^-11 (4 |a| + |b| + |w|) with a margin of 2
    amax = np.abs(f32).max(axis=1, keepdims=True) + 1e-30
    assert np.all(np.abs(got - f32) <= 2 * 2.0 ** -11 * (9 * amax + np.abs(f32)))


# ---------------------------------------------------------------- 2. round trip
# relative RMS error of quantize -> dequantize on 2^16 N(0, 1) samples, measured with seed 0 on
# the quantiser alone:  Q2_K 0.3263   Q3_K 0.1551   (Q4_K measures 0.078 with the same data);
# the bounds are 1.5 x those values, as tests/test_legacy_quants.py
MEASURED = {Q2_K: 0.3263, Q3_K: 0.1551}


@pytest.mark.parametrize("t", NEW)
@pytest.mark.parametrize("seed", [0, 1])
def test_quantize_roundtrip_error(t, seed):
    x = np.random.default_rng(seed).standard_normal(1 << 16).astype(np.float32)
    raw = quantize(x, t)
    assert raw.size == tensor_nbytes(t, x.size)
    y = dequantize(raw, t, x.size)
    rel = float(np.sqrt(np.mean((y - x) ** 2)) / np.sqrt(np.mean(x ** 2)))
    print(t.name, seed, rel)
    assert rel < 1.5 * MEASURED[t], rel
    assert rel > 0.5 * MEASURED[t], rel   # (a quantiser that lost its 2 / 3 bits would not sit here)
    y16 = dequantize(raw, t, x.size, arith="f16")
    assert np.max(np.abs(y16 - y)) <= 2 * 2.0 ** -11 * 10 * np.max(np.abs(y))


@pytest.mark.parametrize("t", NEW)
def test_random_blocks_are_finite(t):
    raw = random_blocks(t, 256 * 512, np.random.default_rng(3), std=0.02)
    assert raw.size == tensor_nbytes(t, 256 * 512)
    w = dequantize(raw, t, 256 * 512)
    assert np.isfinite(w).all()
    assert 0.015 < float(w.std()) < 0.03 and abs(float(w.mean())) < 2e-3


# ---------------------------------------------------------------- 3. synthetic files
MIXES = {"tiny-llama3-q2_k": (10, {Q2_K, Q3_K, GGMLType.Q6_K}),
         "tiny-llama3-q3_k_s": (11, {Q3_K, GGMLType.Q6_K}),
         "tiny-llama3-q3_k_m": (12, {Q3_K, GGMLType.Q4_K, GGMLType.Q5_K, GGMLType.Q6_K})}


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    d = tmp_path_factory.mktemp("k23_models")
    names = list(MIXES) + ["tiny-qwen2-q3_k_m", "tiny-kmixed-1l"]
    return {m: write_synthetic_gguf(m, str(d / f"{m}.gguf")) for m in names}


@pytest.mark.parametrize("name", list(MIXES))
def test_mix_types_and_file_type(paths, name):
    ftype, want_types = MIXES[name]
    spec = SPECS[name]
    rd = GGUFReader(paths[name])
    _, n_vocab = build_vocab(spec)
    plan = tensor_plan(spec, n_vocab)
    seen, total = set(), 0
    for tname, t, shape in plan:
        ti = rd.tensors[tname]
        assert GGMLType(ti.ggml_type) == t, tname
        n = int(np.prod(shape))
        assert np.asarray(rd.raw(tname)).nbytes == tensor_nbytes(t, n), tname
        total += (tensor_nbytes(t, n) + 31) // 32 * 32
        if len(shape) >= 2:
            seen.add(t)
    assert seen == want_types
    assert hparams_metadata(spec, n_vocab)["general.file_type"] == ftype
    assert int(rd.metadata["general.file_type"]) == ftype
    import os
    assert os.path.getsize(paths[name]) - rd.data_offset == total   # tensor_nbytes sums to the data section
    base = Q2_K if name.endswith("q2_k") else Q3_K
    assert GGMLType(rd.tensors["token_embd.weight"].ggml_type) == base
    assert GGMLType(rd.tensors["output.weight"].ggml_type) == GGMLType.Q6_K
    for layer in range(spec.n_layer):
        tt = tensor_types(spec, layer)
        assert tt["attn_q"] == tt["attn_k"] == tt["ffn_gate"] == tt["ffn_up"] == base
        if name.endswith("q3_k_s"):
            assert set(tt.values()) == {Q3_K}
        elif name.endswith("q3_k_m"):
            assert tt["attn_v"] == (GGMLType.Q5_K if layer < 2 else GGMLType.Q4_K)
            assert tt["attn_output"] == GGMLType.Q4_K and tt["ffn_down"] == GGMLType.Q4_K
        else:
            assert tt["attn_v"] == tt["attn_output"] == tt["ffn_down"] == Q3_K


def test_bench_specs_exist():
    assert tensor_types(SPECS["llama3-8b-q3_k_m"], 0)["ffn_down"] == GGMLType.Q5_K   # first n_layer / 16 layers
    assert tensor_types(SPECS["llama3-8b-q3_k_m"], 5)["ffn_down"] == GGMLType.Q4_K
    assert tensor_types(SPECS["llama3-8b-q2_k"], 5)["attn_v"] == GGMLType.Q4_K       # GQA group 4
    assert tensor_types(SPECS["tiny-kmixed-1l"], 0) == {
        "attn_q": Q2_K, "attn_k": Q3_K, "attn_v": GGMLType.Q4_K, "attn_output": GGMLType.Q6_K,
        "ffn_gate": Q2_K, "ffn_up": Q2_K, "ffn_down": Q3_K}
    assert tensor_types(SPECS["tiny-qwen2-q3_k_m"], 0)["attn_q"] == Q3_K and SPECS["tiny-qwen2-q3_k_m"].qkv_bias


@pytest.mark.parametrize("name", list(MIXES))
def test_cpp_reader_reports_the_same_types(paths, name):
    cpu = load_cpu()
    rd = GGUFReader(paths[name])
    got = cpu.gguf_tensor_types(paths[name])
    assert got == {n: int(ti.ggml_type) for n, ti in rd.tensors.items()}


# ---------------------------------------------------------------- 4. planar repack
def _planar_numpy(t, raw, R, K):
    """The layout of csrc/common.h."""
    b = raw.reshape(R, K // 256, BYTES[t])
    if t == Q2_K:
        planes = [b[:, :, 16:80], b[:, :, 0:16], b[:, :, 80:84]]
    else:
        planes = [b[:, :, 32:96], b[:, :, 0:32], b[:, :, 96:108], b[:, :, 108:110]]
    return np.concatenate([p.reshape(-1) for p in planes])


def _repack():
    return load_cpu().repack


@pytest.mark.parametrize("t", NEW)
def test_repack_planar_layout_and_shards(t):
    rng = np.random.default_rng(int(t))
    R, K = 70, 768
    raw = np.frombuffer(rng.bytes(R * (K // 256) * BYTES[t]), np.uint8).copy()
    full = _repack()(int(t), raw, K, 0, R, 0, K, R, 0, 0)
    assert full.size == raw.size   # the planar copy keeps the GGUF byte count
    assert np.array_equal(full, _planar_numpy(t, raw, R, K))
    # TP row shards: two row slices, repacked apart, hold the rows of the whole-matrix repack
    r_split = 32
    for r0, Rs in ((0, r_split), (r_split, R - r_split)):
        rows = raw.reshape(R, -1)[r0:r0 + Rs].reshape(-1)
        part = _repack()(int(t), raw, K, r0, Rs, 0, K, Rs, 0, 0)
        assert np.array_equal(part, _planar_numpy(t, rows, Rs, K))
    # the two slices written into one destination equal the whole repack
    both = _repack()(int(t), raw, K, 0, r_split, 0, K, R, 0, 0) | \
        _repack()(int(t), raw, K, r_split, R - r_split, 0, K, R, 0, r_split)
    assert np.array_equal(both, full)
    # a column shard (whole blocks)
    cols = raw.reshape(R, K // 256, BYTES[t])[:, 1:3].reshape(-1)
    part = _repack()(int(t), raw, K, 0, R, 256, 512, R, 0, 0)
    assert np.array_equal(part, _planar_numpy(t, cols, R, 512))
    with pytest.raises(RuntimeError):
        _repack()(int(t), raw, K, 0, R, 0, 384, R, 0, 0)   # K must be whole 256-weight blocks


@pytest.mark.parametrize("t", NEW)
def test_repack_gate_up_interleave(t):
    rng = np.random.default_rng(50 + int(t))
    F, K = 64, 256
    nbytes = BYTES[t]
    g = np.frombuffer(rng.bytes(F * nbytes), np.uint8).copy()
    u = np.frombuffer(rng.bytes(F * nbytes), np.uint8).copy()
    planar = _repack()(int(t), g, K, 0, F, 0, K, 2 * F, 32, 0) | _repack()(int(t), u, K, 0, F, 0, K, 2 * F, 32, 32)
    rows = np.empty((2 * F, nbytes), np.uint8)
    for f in range(F):
        rows[(f // 32) * 64 + f % 32] = g.reshape(F, nbytes)[f]
        rows[(f // 32) * 64 + 32 + f % 32] = u.reshape(F, nbytes)[f]
    assert np.array_equal(planar, _planar_numpy(t, rows.reshape(-1), 2 * F, K))


# ---------------------------------------------------------------- 5. CPU backend
CPU_MODELS = list(MIXES) + ["tiny-qwen2-q3_k_m", "tiny-kmixed-1l"]


def _rel(a, b):
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-12))


@pytest.mark.parametrize("model", CPU_MODELS)
def test_cpu_prefill_and_decode_logits_match_reference(paths, model):
    """As tests/test_cpu_backend.py::test_prefill_logits_match_reference, with its bound (0.06)."""
    cpu = load_cpu()
    path = paths[model]
    ref = ReferenceLlama(GGUFReader(path), n_ctx=64)
    toks = [int(t) for t in np.random.default_rng(1).integers(3, 500, 20)]
    want = ref.forward(toks, 0).numpy()
    eng = cpu.CpuEngine(path, n_ctx=64, n_threads=4, n_batch=8)
    got = eng.eval_logits(toks, 0)
    assert got.shape == want.shape
    print(model, _rel(got, want))
    assert _rel(got, want) < 0.06, _rel(got, want)
    want2 = ref.forward([7], len(toks)).numpy()
    assert _rel(eng.eval_logits([7], len(toks)), want2) < 0.06


@pytest.mark.parametrize("t", NEW)
def test_cpu_embedding_row(t, paths):
    """token_embd of these files is Q2_K / Q3_K: an engine that runs no layer returns the
    embedding rows as its hidden state."""
    name = "tiny-llama3-q2_k" if t == Q2_K else "tiny-llama3-q3_k_s"
    rd = GGUFReader(paths[name])
    ti = rd.tensors["token_embd.weight"]
    assert GGMLType(ti.ggml_type) == t
    emb = dequantize(np.asarray(rd.raw("token_embd.weight")), t, ti.n_elements).reshape(ti.shape[::-1])
    eng = load_cpu().CpuEngine(paths[name], n_ctx=32, n_threads=2, n_batch=8, layer_end=0, load_head=False)
    ids = [0, 5, 17, emb.shape[0] - 1]
    rows = eng.eval_hidden(ids, 0)
    assert np.allclose(rows, emb[ids], rtol=1e-5, atol=0)


# ---------------------------------------------------------------- 6. MoE experts are refused
def test_k23_expert_tensors_are_refused(tmp_path):
    spec = replace(SPECS["tiny-mixtral-q4_k_m"], name="tiny-mixtral-q3_k_s", quant="q3_k_s")
    path = write_synthetic_gguf(spec, str(tmp_path / "moe.gguf"))
    with pytest.raises(RuntimeError, match=r"ffn_(gate|up|down)_exps\.weight.*Q3_K"):
        load_cpu().CpuEngine(path, n_ctx=64, n_threads=2, n_batch=8)
