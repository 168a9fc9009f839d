"""The non-linear 4-bit pair (IQ4_NL, IQ4_XS) without a GPU: the NumPy reference against blocks
built by hand from the format's formulas, the quantiser's fixed point, the synthetic mixes, the
planar repack and the C++ CPU backend."""
from dataclasses import replace

import numpy as np
import pytest

from llama_fastapi_k8s_gpu_amd.gguf.constants import (FTYPE_MOSTLY_IQ4_NL, FTYPE_MOSTLY_IQ4_XS, GGML_BLOCK,
                                                      GGMLType, tensor_nbytes)
from llama_fastapi_k8s_gpu_amd.gguf.quants import dequantize, quantize, random_blocks
from llama_fastapi_k8s_gpu_amd.gguf.reader import GGUFReader
from llama_fastapi_k8s_gpu_amd.gguf.synthetic import SPECS, tensor_types, write_synthetic_gguf
from llama_fastapi_k8s_gpu_amd.models.llama import ReferenceLlama
from llama_fastapi_k8s_gpu_amd.runtime import load_cpu

IQ4_NL, IQ4_XS = GGMLType.IQ4_NL, GGMLType.IQ4_XS
NEW = [IQ4_NL, IQ4_XS]
BLOCK = {IQ4_NL: (32, 18), IQ4_XS: (256, 136)}
KVALUES = [-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113]


def _f16(b):
    return np.float32(np.frombuffer(bytes(b), dtype="<f2")[0])


def formula_iq4_nl(blk):
    """The 32 weights of one IQ4_NL block, weight by weight from the format's formulas."""
    blk = bytes(blk)
    d, qs = _f16(blk[0:2]), blk[2:18]
    out = np.empty(32, np.float32)
    for j in range(16):
        out[j] = d * np.float32(KVALUES[qs[j] & 15])
        out[j + 16] = d * np.float32(KVALUES[qs[j] >> 4])
    return out


def iq4_xs_ls(blk):
    blk = bytes(blk)
    scales_h = blk[2] | (blk[3] << 8)
    scales_l = blk[4:8]
    return [((scales_l[ib // 2] >> (4 * (ib % 2))) & 15) | (((scales_h >> (2 * ib)) & 3) << 4) for ib in range(8)]


def formula_iq4_xs(blk):
    blk = bytes(blk)
    d, qs = _f16(blk[0:2]), blk[8:136]
    ls = iq4_xs_ls(blk)
    out = np.empty(256, np.float32)
    for ib in range(8):
        dl = d * np.float32(ls[ib] - 32)
        for j in range(16):
            q = qs[16 * ib + j]
            out[32 * ib + j] = dl * np.float32(KVALUES[q & 15])
            out[32 * ib + 16 + j] = dl * np.float32(KVALUES[q >> 4])
    return out


FORMULA = {IQ4_NL: formula_iq4_nl, IQ4_XS: formula_iq4_xs}


def _random_blocks_finite(t, nb, rng):
    bb = BLOCK[t][1]
    raw = np.frombuffer(rng.bytes(nb * bb), np.uint8).reshape(nb, bb).copy()
    raw[:, 0:2] = rng.uniform(-2.0, 2.0, nb).astype(np.float16).reshape(-1, 1).view(np.uint8)
    return raw


def _iq4_xs_block(d, ls, qs):
    scales_h, scales_l = 0, bytearray(4)
    for ib, v in enumerate(ls):
        scales_l[ib // 2] |= (v & 15) << (4 * (ib % 2))
        scales_h |= (v >> 4) << (2 * ib)
    blk = np.float16(d).tobytes() + bytes([scales_h & 0xFF, scales_h >> 8]) + bytes(scales_l) + bytes(qs)
    assert len(blk) == 136
    return blk


# ---------------------------------------------------------------- 1. format exactness
@pytest.mark.parametrize("t", NEW)
def test_block_sizes(t):
    assert GGML_BLOCK[t] == BLOCK[t]
    bs, bb = BLOCK[t]
    assert tensor_nbytes(t, bs * 7) == 7 * bb
    assert tensor_nbytes(IQ4_NL, 32) == 18 and tensor_nbytes(IQ4_XS, 256) == 136
    assert (int(IQ4_NL), int(IQ4_XS)) == (20, 23)
    assert (FTYPE_MOSTLY_IQ4_NL, FTYPE_MOSTLY_IQ4_XS) == (25, 30)


def test_iq4_nl_one_block_by_hand():
    qs = bytes((i | ((15 - i) << 4)) for i in range(16))   # every index once in each nibble
    blk = np.float16(-0.375).tobytes() + qs
    got = dequantize(np.frombuffer(blk, np.uint8), IQ4_NL, 32)
    assert got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), formula_iq4_nl(blk).view(np.uint32))
    for j in range(16):
        assert got[j] == np.float32(-0.375 * KVALUES[j])            # the low nibbles: weights 0..15
        assert got[16 + j] == np.float32(-0.375 * KVALUES[15 - j])  # the high nibbles: weights 16..31


def test_iq4_xs_one_block_by_hand():
    """ls = 0, 31, 32 and 63, both nibbles of every scales_l byte and every bit pair of scales_h."""
    ls = [0, 31, 32, 63, 17, 46, 5, 58]
    assert {v >> 4 for v in ls} == {0, 1, 2, 3}
    qs = bytes((37 * b + 11) & 0xFF for b in range(128))
    blk = _iq4_xs_block(0.75, ls, qs)
    assert iq4_xs_ls(blk) == ls
    got = dequantize(np.frombuffer(blk, np.uint8), IQ4_XS, 256)
    assert got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), formula_iq4_xs(blk).view(np.uint32))
    # spot values written out: weight 0, weight 16 (high nibble of byte 0) and weight 255
    assert got[0] == np.float32(0.75 * (0 - 32) * KVALUES[11 & 15])
    assert got[16] == np.float32(0.75 * (0 - 32) * KVALUES[11 >> 4])
    assert got[255] == np.float32(0.75 * (58 - 32) * KVALUES[qs[127] >> 4])
    assert np.all(got[64:96] == 0)                                   # ls = 32: the sub-block is zero
    assert got[32 + 3] == np.float32(0.75 * -1 * KVALUES[qs[16 + 3] & 15])   # ls = 31
    assert got[96 + 20] == np.float32(0.75 * 31 * KVALUES[qs[48 + 4] >> 4])  # ls = 63
    # every ls pattern in every position
    for shift in range(8):
        ls2 = ls[shift:] + ls[:shift]
        blk2 = _iq4_xs_block(-1.5, ls2, qs)
        got2 = dequantize(np.frombuffer(blk2, np.uint8), IQ4_XS, 256)
        assert np.array_equal(got2.view(np.uint32), formula_iq4_xs(blk2).view(np.uint32))


@pytest.mark.parametrize("t", NEW)
def test_dequantize_equals_formula(t):
    rng = np.random.default_rng(100 + int(t))
    bs = BLOCK[t][0]
    raw = _random_blocks_finite(t, 24, rng)
    got = dequantize(raw.reshape(-1), t, 24 * bs).reshape(24, bs)
    want = np.stack([FORMULA[t](raw[i]) for i in range(24)])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("t", NEW)
def test_f16_arithmetic_is_one_rounding(t):
    """arith="f16": the sub-block scale is f16(d * (ls - 32)) (IQ4_NL: d) and every weight is ONE f16
    rounding of codebook value * scale."""
    rng = np.random.default_rng(7 + int(t))
    bs = BLOCK[t][0]
    raw = _random_blocks_finite(t, 24, rng)
    got = dequantize(raw.reshape(-1), t, 24 * bs, arith="f16").reshape(24, bs)
    f32 = dequantize(raw.reshape(-1), t, 24 * bs).reshape(24, bs)
    for i in range(24):
        blk = bytes(raw[i])
        d = _f16(blk[0:2])
        if t == IQ4_NL:
            a, qs = [np.float64(d)], blk[2:18]
        else:
            a, qs = [np.float64(np.float16(d * np.float32(v - 32))) for v in iq4_xs_ls(blk)], blk[8:136]
        want = np.empty(bs, np.float64)
        for ib in range(bs // 32):
            for j in range(16):
                want[32 * ib + j] = KVALUES[qs[16 * ib + j] & 15] * a[ib]
                want[32 * ib + 16 + j] = KVALUES[qs[16 * ib + j] >> 4] * a[ib]
        assert np.array_equal(got[i], want.astype(np.float16).astype(np.float32)), i
    # the scale and the result each round once (2^-11 relative), with a margin of 2
    assert np.all(np.abs(got - f32) <= 2 * 2.0 ** -11 * 2 * np.abs(f32))


# ---------------------------------------------------------------- 2. quantiser, random blocks
@pytest.mark.parametrize("t", NEW)
@pytest.mark.parametrize("seed,scale", [(0, 1.0), (1, 0.02), (2, 37.0)])
def test_quantize_dequantize_is_a_fixed_point(t, seed, scale):
    x = np.random.default_rng(seed).standard_normal(1 << 14).astype(np.float32) * np.float32(scale)
    x[512:768] = 0.0          # an all-zero block
    x[1024:1056] = 0.0        # an all-zero sub-block
    x[2048] = 1000.0 * scale  # one sub-block far above the others: their scales truncate to small ls
    raw = quantize(x, t)
    assert raw.dtype == np.uint8 and raw.size == tensor_nbytes(t, x.size)
    y = dequantize(raw, t, x.size)
    assert np.isfinite(y).all()
    raw2 = quantize(y, t)
    assert np.array_equal(raw2, raw)
    assert np.array_equal(dequantize(raw2, t, x.size), y)
    # nearest codebook entry around a scale taken from the extreme weight: 4-bit quality on the plain blocks
    rel = float(np.sqrt(np.mean((y[4096:] - x[4096:]) ** 2)) / np.sqrt(np.mean(x[4096:] ** 2)))
    print(t.name, seed, rel)
    assert rel < 0.15, rel


@pytest.mark.parametrize("t", NEW)
def test_random_blocks_are_finite(t):
    raw = random_blocks(t, 256 * 512, np.random.default_rng(3), std=0.02)
    assert raw.size == tensor_nbytes(t, 256 * 512)
    w = dequantize(raw, t, 256 * 512)
    assert np.isfinite(w).all()
    assert 0.015 < float(w.std()) < 0.03 and abs(float(w.mean())) < 2e-3


# ---------------------------------------------------------------- 3. synthetic files
def test_specs_and_mix():
    for name, base in (("tiny-llama3-iq4_xs", IQ4_XS), ("tiny-llama3-iq4_nl", IQ4_NL)):
        spec = SPECS[name]
        for layer in range(spec.n_layer):
            tt = tensor_types(spec, layer)
            assert tt["attn_q"] == tt["attn_k"] == tt["attn_output"] == tt["ffn_gate"] == tt["ffn_up"] == base
            assert tt["attn_v"] == base                      # GQA group 2
            assert tt["ffn_down"] == (GGMLType.Q5_K if layer < spec.n_layer // 8 else base)
    big = SPECS["llama3-8b-iq4_xs"]
    assert tensor_types(big, 0)["attn_v"] == GGMLType.Q5_K   # GQA group 4
    assert tensor_types(big, 3)["ffn_down"] == GGMLType.Q5_K and tensor_types(big, 4)["ffn_down"] == IQ4_XS
    assert tensor_types(SPECS["tiny-iq4-mixed"], 0) == {
        "attn_q": IQ4_NL, "attn_k": IQ4_XS, "attn_v": GGMLType.Q4_K, "attn_output": GGMLType.Q6_K,
        "ffn_gate": IQ4_NL, "ffn_up": IQ4_NL, "ffn_down": IQ4_XS}
    assert SPECS["tiny-qwen2-iq4_xs"].qkv_bias and tensor_types(SPECS["tiny-qwen2-iq4_xs"], 0)["attn_q"] == IQ4_XS
    odd = SPECS["tiny-iq4_nl-oddff"]
    assert odd.n_ff % 32 == 0 and odd.n_ff % 256 != 0 and tensor_types(odd, 0)["ffn_down"] == IQ4_NL


CPU_MODELS = ["tiny-llama3-iq4_xs", "tiny-llama3-iq4_nl", "tiny-iq4-mixed", "tiny-iq4_nl-oddff"]


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    d = tmp_path_factory.mktemp("iq4_models")
    return {m: write_synthetic_gguf(m, str(d / f"{m}.gguf")) for m in CPU_MODELS}


@pytest.mark.parametrize("name,ftype,base", [("tiny-llama3-iq4_xs", 30, IQ4_XS), ("tiny-llama3-iq4_nl", 25, IQ4_NL)])
def test_file_types_and_both_readers(paths, name, ftype, base):
    rd = GGUFReader(paths[name])
    assert int(rd.metadata["general.file_type"]) == ftype
    assert GGMLType(rd.tensors["token_embd.weight"].ggml_type) == base
    assert GGMLType(rd.tensors["output.weight"].ggml_type) == GGMLType.Q6_K
    assert GGMLType(rd.tensors["blk.1.attn_q.weight"].ggml_type) == base
    got = load_cpu().gguf_tensor_types(paths[name])
    assert got == {n: int(ti.ggml_type) for n, ti in rd.tensors.items()}


# ---------------------------------------------------------------- 4. planar repack
def _decode_planar(t, planar, R, K):
    """Weights [R, K] from the planar layout of csrc/common.h, decoded from its planes."""
    kv = np.array(KVALUES, np.float32)
    nb = K // 32
    qs = planar[:R * nb * 16].reshape(R, nb, 16)
    rest = planar[R * nb * 16:]
    idx = np.concatenate([qs & 15, qs >> 4], axis=2)          # [R, chunk, 32]: Q4_0's nibble order
    if t == IQ4_NL:
        scale = rest.view("<f2").astype(np.float32).reshape(R, nb)
    else:
        sc = rest.reshape(R, K // 256, 8)                      # d | scales_h | scales_l[4] as they stand
        d = sc[:, :, 0:2].copy().view("<f2").astype(np.float32)[:, :, 0]
        sh = sc[:, :, 2].astype(np.int32) | (sc[:, :, 3].astype(np.int32) << 8)
        scale = np.empty((R, K // 256, 8), np.float32)
        for ib in range(8):
            ls = ((sc[:, :, 4 + ib // 2] >> (4 * (ib % 2))) & 15).astype(np.int32) | (((sh >> (2 * ib)) & 3) << 4)
            scale[:, :, ib] = d * (ls - 32).astype(np.float32)
        scale = scale.reshape(R, nb)
    return (scale[:, :, None] * kv[idx]).reshape(R, K)


@pytest.mark.parametrize("t,R,K", [(IQ4_NL, 5, 256), (IQ4_NL, 3, 768), (IQ4_NL, 7, 96),
                                   (IQ4_XS, 5, 256), (IQ4_XS, 3, 768)])
def test_repack_planes_decode_to_the_reference(t, R, K):
    rng = np.random.default_rng(int(t) + K)
    bs, bb = BLOCK[t]
    raw = _random_blocks_finite(t, R * K // bs, rng).reshape(-1)
    planar = load_cpu().repack(int(t), raw, K, 0, R, 0, K, R, 0, 0)
    assert planar.size == raw.size   # the planar copy keeps the GGUF byte count
    want = dequantize(raw, t, R * K).reshape(R, K)
    got = _decode_planar(t, np.asarray(planar), R, K)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # plane alignment: the scale plane starts on a 16-byte boundary
    assert (R * (K // 32) * 16) % 16 == 0
    if R > 3:   # a row shard repacked apart holds the rows of the whole-matrix repack
        part = load_cpu().repack(int(t), raw, K, 2, R - 2, 0, K, R - 2, 0, 0)
        assert np.array_equal(_decode_planar(t, np.asarray(part), R - 2, K), want[2:])


# ---------------------------------------------------------------- 5. CPU backend
def _rel(a, b):
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-12))


@pytest.mark.parametrize("model", CPU_MODELS)
def test_cpu_prefill_and_decode_logits_match_reference(paths, model):
    """As tests/test_kquants_23.py's test of the same name, with its bound (0.06): the fp32 torch
    reference model loads the same file through the NumPy dequantisation."""
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


@pytest.mark.parametrize("name,t", [("tiny-llama3-iq4_nl", IQ4_NL), ("tiny-llama3-iq4_xs", IQ4_XS)])
def test_cpu_embedding_row(paths, name, t):
    """token_embd of these files has the base type: an engine that runs no layer returns the
    embedding rows as its hidden state."""
    rd = GGUFReader(paths[name])
    ti = rd.tensors["token_embd.weight"]
    assert GGMLType(ti.ggml_type) == t
    emb = dequantize(np.asarray(rd.raw("token_embd.weight")), t, ti.n_elements).reshape(ti.shape[::-1])
    eng = load_cpu().CpuEngine(paths[name], n_ctx=32, n_threads=2, n_batch=8, layer_end=0, load_head=False)
    ids = [0, 5, 17, emb.shape[0] - 1]
    assert np.allclose(eng.eval_hidden(ids, 0), emb[ids], rtol=1e-5, atol=0)


# ---------------------------------------------------------------- 6. refusals
def test_iq4_xs_needs_whole_256_blocks():
    """K = 288 is nine IQ4_NL blocks but no whole number of IQ4_XS blocks."""
    repack = load_cpu().repack
    raw = np.zeros(2 * 136, np.uint8)
    with pytest.raises(RuntimeError, match="multiple of the type's block size"):
        repack(int(IQ4_XS), raw, 288, 0, 1, 0, 288, 1, 0, 0)
    nl = repack(int(IQ4_NL), np.zeros(9 * 18, np.uint8), 288, 0, 1, 0, 288, 1, 0, 0)
    assert nl.size == 9 * 18


def test_iq4_expert_tensors_are_refused(tmp_path):
    spec = replace(SPECS["tiny-mixtral-q4_k_m"], name="tiny-mixtral-iq4_xs", quant="iq4_xs")
    path = write_synthetic_gguf(spec, str(tmp_path / "moe.gguf"))
    with pytest.raises(RuntimeError, match=r"ffn_(gate|up|down)_exps\.weight.*IQ4_XS"):
        load_cpu().CpuEngine(path, n_ctx=64, n_threads=2, n_batch=8)


@pytest.mark.parametrize("tid", [21, 22])
def test_neighbouring_type_ids_stay_unsupported(tid):
    """ggml types 21 and 22 (between IQ4_NL = 20 and IQ4_XS = 23) are other formats."""
    with pytest.raises(RuntimeError, match="unsupported ggml type"):
        load_cpu().repack(tid, np.zeros(256, np.uint8), 256, 0, 1, 0, 256, 1, 0, 0)
    with pytest.raises(ValueError):
        GGMLType(tid)
