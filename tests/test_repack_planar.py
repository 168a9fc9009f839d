"""The planar repack of Q4_K, Q5_K, Q6_K, Q8_0, F16, BF16 and F32, byte for byte, without a GPU
(the legacy, Q2_K / Q3_K and IQ4 types have theirs in test_legacy_quants.py, test_kquants_23.py and
test_iq4.py). The slices below are written out from the GGUF block definitions, not read from the
C++ layout table, so the two descriptions stay independent."""
import numpy as np
import pytest

from llama_fastapi_k8s_gpu_amd.gguf.constants import GGML_BLOCK, GGMLType
from llama_fastapi_k8s_gpu_amd.runtime import load_cpu

T = GGMLType
TYPES = [T.Q4_K, T.Q5_K, T.Q6_K, T.Q8_0, T.F16, T.BF16, T.F32]
# (weights per block, bytes per block, K of the test, column shard [c0, c1))
SHAPE = {
    T.Q4_K: (256, 144, 768, 256, 768),
    T.Q5_K: (256, 176, 768, 256, 768),
    T.Q6_K: (256, 210, 768, 256, 768),
    T.Q8_0: (32, 34, 96, 32, 96),
    T.F16: (1, 2, 24, 8, 24),
    T.BF16: (1, 2, 24, 8, 24),
    T.F32: (1, 4, 24, 8, 24),
}
R = 70


def _planar_numpy(t, raw, rows, K):
    """The layout of csrc/common.h: one plane per GGUF field, each [rows][K / block][field bytes]."""
    block, nbytes = SHAPE[t][:2]
    b = raw.reshape(rows, K // block, nbytes)
    if t == T.Q4_K:    # GGUF: d, dmin, scales[12] | qs[128]
        planes = [b[:, :, 16:144], b[:, :, 0:16]]
    elif t == T.Q5_K:  # GGUF: d, dmin, scales[12] | qh[32] | qs[128]
        planes = [b[:, :, 48:176], b[:, :, 16:48], b[:, :, 0:16]]
    elif t == T.Q6_K:  # GGUF: ql[128] | qh[64] | scales[16] | d
        planes = [b[:, :, 0:128], b[:, :, 128:192], b[:, :, 192:208], b[:, :, 208:210]]
    elif t == T.Q8_0:  # GGUF: d | qs[32]
        planes = [b[:, :, 2:34], b[:, :, 0:2]]
    else:              # F16 / BF16 / F32: [rows][K] unchanged
        planes = [b]
    return np.concatenate([p.reshape(-1) for p in planes])


def _repack():
    return load_cpu().repack


def _random(rng, t, rows, K):
    block, nbytes = SHAPE[t][:2]
    return np.frombuffer(rng.bytes(rows * (K // block) * nbytes), np.uint8).copy()


def test_shapes_agree_with_the_python_block_table():
    for t in TYPES:
        assert GGML_BLOCK[t] == SHAPE[t][:2]


@pytest.mark.parametrize("t", TYPES)
def test_repack_planar_layout_and_shards(t):
    rng = np.random.default_rng(int(t))
    block, nbytes, K, c0, c1 = SHAPE[t]
    raw = _random(rng, t, R, K)
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
    cols = raw.reshape(R, K // block, nbytes)[:, c0 // block:c1 // block].reshape(-1)
    part = _repack()(int(t), raw, K, 0, R, c0, c1 - c0, R, 0, 0)
    assert np.array_equal(part, _planar_numpy(t, cols, R, c1 - c0))


@pytest.mark.parametrize("t", TYPES)
def test_repack_gate_up_interleave(t):
    rng = np.random.default_rng(50 + int(t))
    block, nbytes, K = SHAPE[t][:3]
    F = 64
    row_bytes = (K // block) * nbytes
    g = _random(rng, t, F, K)
    u = _random(rng, t, F, K)
    planar = _repack()(int(t), g, K, 0, F, 0, K, 2 * F, 32, 0) | _repack()(int(t), u, K, 0, F, 0, K, 2 * F, 32, 32)
    # destination rows: 32 gate rows, then the 32 up rows of the same features, and so on
    rows = np.empty((2 * F, row_bytes), np.uint8)
    for f in range(F):
        rows[(f // 32) * 64 + f % 32] = g.reshape(F, row_bytes)[f]
        rows[(f // 32) * 64 + 32 + f % 32] = u.reshape(F, row_bytes)[f]
    assert np.array_equal(planar, _planar_numpy(t, rows.reshape(-1), 2 * F, K))


# F16 / BF16 / F32 have one-weight blocks: every K is aligned, so only the block types can refuse
@pytest.mark.parametrize("t", [T.Q4_K, T.Q5_K, T.Q6_K, T.Q8_0])
def test_repack_refuses_an_unaligned_k(t):
    block, _, K = SHAPE[t][:3]
    raw = _random(np.random.default_rng(0), t, R, K)
    with pytest.raises(RuntimeError, match="multiple of the type's block size"):
        _repack()(int(t), raw, K, 0, R, 0, K - block // 2, R, 0, 0)   # a slice that ends inside a block
    with pytest.raises(RuntimeError, match="unaligned column slice"):
        _repack()(int(t), raw, K, 0, R, block // 2, block, R, 0, 0)   # a slice that starts inside one
