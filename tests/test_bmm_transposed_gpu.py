"""The wave-owned batched projections in both tile orientations (BmmArgs::tr, the bindings' `tr`):
tr = 0 keeps the weights as the MFMA's A operand - C[weight row 4kq + i][activation column r16] -
and tr = 1 swaps the operands - C[activation row 4kq + i][weight row r16] - so that every split-K
add covers whole 64-byte segments of one activation row. A swapped row / column or an unmasked lane
of the transposed epilogue lands in the padding this file puts around every output."""
import functools

import numpy as np
import pytest

from llama_fastapi_k8s_gpu_amd.gguf.constants import GGMLType
from llama_fastapi_k8s_gpu_amd.gguf.quants import random_blocks
from gpu_helpers import dev_bytes, hip, make_matrix, rel_err, stream, to_planar

pytestmark = pytest.mark.gpu

Q4, Q6 = GGMLType.Q4_K, GGMLType.Q6_K


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _swizzle4(x):
    """bprep's k order inside each 4-group: (0, 2, 1, 3)."""
    return x.reshape(*x.shape[:-1], -1, 4)[..., [0, 2, 1, 3]].reshape(x.shape)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _tile16(t, R, K, seed, swiglu=False, ref=True):
    """(tile16 copy on the device, dequantised float64 [R][K] if `ref`) of one random matrix: built
    once, read-only."""
    import torch
    rng = np.random.default_rng(seed)
    raw, W = make_matrix(t, R, K, rng) if ref else (random_blocks(t, R * K, rng, std=0.05), None)
    dw = dev_bytes(to_planar(t, raw, R, K))
    tw = torch.empty(hip().t16_bytes(int(t), R, K), dtype=torch.uint8, device="cuda")
    hip().t16_repack(dw.data_ptr(), int(t), R, K, tw.data_ptr(), stream(), swiglu=swiglu)
    torch.cuda.synchronize()
    return tw, W.astype(np.float64) if ref else None


@pytest.mark.parametrize("t", [Q4, Q6])
@pytest.mark.parametrize("K", [256, 1024, 4096])   # one part (read-modify-write), two parts, eight parts
@pytest.mark.parametrize("R", [16, 40, 130])       # a whole tile, a half tile, a ragged last tile
@pytest.mark.parametrize("B", [1, 2, 4, 5, 6, 8])  # the activation row is 4 kq + i: 4 | 5 and 8 are its edges
def test_bmm_splitk_both_orientations(torch, t, K, R, B):
    """out[b] += W x[b] against the fp64 product of the f16 activations and the dequantised weights
    (test_bmm_rows_vs_fp32's reference and tolerance), in both orientations, into a buffer of B + 2
    rows with a pitch of R + 6 pre-filled with random values: the partials accumulate onto the
    pre-fill, the padding columns and the extra rows stay bit-unchanged. At K = 256 (one part: no
    atomics, one fixed summation order inside the MFMA chain) the two orientations agree bit for bit."""
    tw, W = _tile16(t, R, K, 1000 * R + K + int(t))
    rng = np.random.default_rng(B * 1000 + R + K + int(t))
    Xh = rng.standard_normal((B, K)).astype(np.float32).astype(np.float16)
    dxh = torch.from_numpy(_swizzle4(Xh)).cuda()
    ldo = R + 6
    y0 = rng.standard_normal((B + 2, ldo)).astype(np.float32)
    ref = Xh.astype(np.float64) @ W.T
    got = {}
    for tr in (0, 1):
        out = torch.from_numpy(y0).cuda()
        hip().bmm(tw.data_ptr(), int(t), R, K, dxh.data_ptr(), K, out.data_ptr(), ldo, B, stream(), tr=tr)
        torch.cuda.synchronize()
        g = got[tr] = out.cpu().numpy()
        for b in range(B):
            e = rel_err(g[b, :R] - y0[b, :R], ref[b])
            assert e < 2e-3, (tr, b, e)
        assert np.array_equal(_bits(g[:B, R:]), _bits(y0[:B, R:])), (tr, "padding columns")
        assert np.array_equal(_bits(g[B:]), _bits(y0[B:])), (tr, "rows past B")
    if K == 256:
        assert np.array_equal(_bits(got[0]), _bits(got[1]))


def _rope_table(n_ctx, hd, theta=5e5):
    inv = theta ** (-np.arange(0, hd, 2, dtype=np.float64) / hd)
    ang = np.arange(n_ctx, dtype=np.float64)[:, None] * inv[None, :]
    return np.stack([np.cos(ang), np.sin(ang)], -1).astype(np.float32)   # [n_ctx][hd/2][2]


def _rope_pairs(y, pos, tab):
    """RoPE on adjacent pairs of y [rows] at position pos, rows % hd per head."""
    hd2 = tab.shape[1]
    z = y.reshape(-1, hd2, 2).astype(np.float64)
    c, s = tab[pos, :, 0].astype(np.float64), tab[pos, :, 1].astype(np.float64)
    return np.stack([z[..., 0] * c - z[..., 1] * s, z[..., 0] * s + z[..., 1] * c], -1).reshape(y.shape)


def _attn_ref(q, K, V, L, scale):
    H, D = q.shape
    G = H // K.shape[0]
    out = np.zeros((H, D))
    for h in range(H):
        k = K[h // G, :L].astype(np.float64)
        s = k @ q[h].astype(np.float64) * scale
        p = np.exp(s - s.max())
        p /= p.sum()
        out[h] = p @ V[h // G, :L].astype(np.float64)
    return out


@pytest.mark.parametrize("types", [(Q4, Q4, Q4), (Q4, Q4, Q6)])   # one run (bmm_sk), two runs (bmm_wt2)
@pytest.mark.parametrize("B", [4, 5, 6])
@pytest.mark.parametrize("tr", [0, 1])
def test_bmm_qkv_splitk_then_attention_both_orientations(torch, types, B, tr):
    """test_bmm_qkv_splitk_then_attention's two stages and tolerances at head_dim 128, 4 query / 2 kv
    heads, K = 1024, with the split-K Q|K|V in either orientation; the two rows behind the B
    accumulation rows stay bit-unchanged."""
    hd, H, Hkv, K = 128, 4, 2, 1024
    tq, tk, tv = types
    assert hip().bmm_qkv_sk_supported(int(tq), int(tk), int(tv), K, B)
    n_ctx, nq, nkv = 256, H * hd, Hkv * hd
    mats = [_tile16(t, R, K, 77 + i + int(t)) for i, (t, R) in enumerate(((tq, nq), (tk, nkv), (tv, nkv)))]
    rng = np.random.default_rng(B * 31 + int(tv))
    X = (rng.standard_normal((B, K)) * 3).astype(np.float32)
    nw = (0.5 + rng.random(K)).astype(np.float32)
    eps = 1e-5
    tab = _rope_table(n_ctx, hd)
    pos = rng.integers(1, n_ctx, B).astype(np.int32)
    slots = rng.permutation(8)[:B].astype(np.int32)
    ldo = nq + 2 * nkv
    dx, dn = torch.from_numpy(X).cuda(), torch.from_numpy(nw).cuda()
    dtab, dpos, dslots = torch.from_numpy(tab).cuda(), torch.from_numpy(pos).cuda(), torch.from_numpy(slots).cuda()
    dfreq = torch.from_numpy((5e5 ** (-np.arange(0, hd, 2, dtype=np.float64) / hd)).astype(np.float32)).cuda()
    guard = rng.standard_normal((2, ldo)).astype(np.float32)
    out = torch.zeros(B + 2, ldo, device="cuda")
    out[B:] = torch.from_numpy(guard).cuda()
    ss = torch.zeros(16, device="cuda")
    hip().bmm_qkv_sk(mats[0][0].data_ptr(), int(tq), nq, mats[1][0].data_ptr(), int(tk), mats[2][0].data_ptr(), int(tv),
                     nkv, K, dx.data_ptr(), K, dn.data_ptr(), eps, B, out.data_ptr(), ldo, ss.data_ptr(),
                     dpos.data_ptr(), dtab.data_ptr(), hd, n_ctx, stream(), tr=tr)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(_bits(got[B:]), _bits(guard))
    got = got.astype(np.float64)
    xw = (X * nw).astype(np.float16).astype(np.float64)
    ss_ref = (X.astype(np.float64) ** 2).sum(1)
    assert np.allclose(ss.cpu().numpy()[:B], ss_ref, rtol=1e-5)
    deferred = hip().bmm_qkv_sk_defers_rope()   # the interleaved-step kernels leave the sums un-RoPE'd
    raw_ref = []
    for b in range(B):
        q = _rope_pairs(xw[b] @ mats[0][1].T, pos[b], tab)
        k = _rope_pairs(xw[b] @ mats[1][1].T, pos[b], tab)
        v = xw[b] @ mats[2][1].T
        qg, kg = got[b, :nq], got[b, nq:nq + nkv]
        if deferred:
            qg, kg = _rope_pairs(qg, pos[b], tab), _rope_pairs(kg, pos[b], tab)
        for name, g, r in (("q", qg, q), ("k", kg, k), ("v", got[b, nq + nkv:], v)):
            assert rel_err(g, r) < 3e-3, (b, name, rel_err(g, r))
        raw_ref.append((q, k, v))
    # stage 2: the batched attention over the raw sums
    slot_stride = Hkv * n_ctx * hd
    Kc = rng.standard_normal((8, Hkv, n_ctx, hd)).astype(np.float16)
    Vc = rng.standard_normal((8, Hkv, n_ctx, hd)).astype(np.float16)
    dK, dV = torch.from_numpy(Kc).cuda(), torch.from_numpy(Vc).cuda()
    part = torch.zeros(B * hip().attn_decode_workspace_floats(n_ctx, H, hd), device="cuda")
    cnt = torch.zeros(64 * B, dtype=torch.int32, device="cuda")
    aout = torch.zeros(B, nq, device="cuda")
    aouth = torch.zeros(B, nq, dtype=torch.float16, device="cuda")
    scale = 1 / np.sqrt(hd)
    hip().attn_decode(out.data_ptr(), dK.data_ptr(), dV.data_ptr(), dpos.data_ptr(), n_ctx, H, Hkv, hd, scale,
                      part.data_ptr(), aout.data_ptr(), stream(), cnt.data_ptr(), batch=B, slots=dslots.data_ptr(),
                      slot_stride=slot_stride, out_h=aouth.data_ptr(), qkv_raw=out.data_ptr(), qkv_ld=ldo, k_off=nq,
                      v_off=nq + nkv, ss=ss.data_ptr(), inv_k=1.0 / K, eps=eps,
                      rope_freq=dfreq.data_ptr() if deferred else 0)
    torch.cuda.synchronize()
    Kg, Vg, ao = dK.cpu().numpy(), dV.cpu().numpy(), aout.cpu().numpy()
    for b in range(B):
        q, k, v = raw_ref[b]
        rs = 1.0 / np.sqrt(ss_ref[b] / K + eps)
        kn = (k * rs).astype(np.float16).reshape(Hkv, hd)
        vn = (v * rs).astype(np.float16).reshape(Hkv, hd)
        s, p = slots[b], pos[b]
        assert rel_err(Kg[s, :, p].astype(np.float64), kn.astype(np.float64)) < 3e-3
        assert rel_err(Vg[s, :, p].astype(np.float64), vn.astype(np.float64)) < 3e-3
        Kr, Vr = Kc[s].copy(), Vc[s].copy()
        Kr[:, p], Vr[:, p] = kn, vn
        ref = _attn_ref((q * rs).reshape(H, hd), Kr, Vr, p + 1, scale)
        assert rel_err(ao[b].reshape(H, hd), ref) < 5e-3, (b, rel_err(ao[b].reshape(H, hd), ref))
    for s in (s for s in range(8) if s not in set(slots.tolist())):
        assert np.array_equal(Kg[s], Kc[s]) and np.array_equal(Vg[s], Vc[s])
    assert int(cnt.abs().sum()) == 0


# the chains on the 8B's d_model with a quarter-width FFN: Wo 256 tiles x 8 K parts, gate/up 512
# tiles, down 256 tiles x 8 K parts of 2 steps - every role and counter of the full shape
CH_F, CH_K = 4096, 4096


@pytest.mark.parametrize("td", [Q4, Q6])
@pytest.mark.parametrize("B", [5, 6])
@pytest.mark.parametrize("tr", [0, 1])
def test_bmm_ffn_chain_both_orientations(torch, td, B, tr):
    """bmm_ffn_chain (gate/up + down in one launch) with its down role in either orientation against
    the two separate launches (the down at tr = 0), at test_bmm_ffn_chain_matches_two_launches'
    tolerances: the SwiGLU rows bit-identical, the down sums equal up to the atomics' order."""
    F, K = CH_F, CH_K
    tg, _ = _tile16(Q4, 2 * F, K, 501, True, False)
    tdw, _ = _tile16(td, K, F, 502 + int(td), False, False)
    rng = np.random.default_rng(B * 10 + int(td))
    X = rng.standard_normal((B, K)).astype(np.float32)
    dxf = torch.from_numpy(X * 3).cuda()
    dxh = torch.zeros(B, K, dtype=torch.float16, device="cuda")   # (unused: the norm path stages dxf)
    nw = torch.from_numpy((0.5 + rng.random(K)).astype(np.float32)).cuda()
    resid = torch.from_numpy(rng.standard_normal((B, K)).astype(np.float32)).cuda()
    h_ref = torch.zeros(B, F, dtype=torch.float16, device="cuda")
    out_ref = resid.clone()
    hip().bmm(tg.data_ptr(), int(Q4), 2 * F, K, dxh.data_ptr(), K, 0, 0, B, stream(),
              h_out=h_ref.data_ptr(), ldh_out=F, xf=dxf.data_ptr(), ldxf=K, norm=nw.data_ptr(), eps=1e-5)
    hip().bmm(tdw.data_ptr(), int(td), K, F, h_ref.data_ptr(), F, out_ref.data_ptr(), K, B, stream(), tr=0)
    torch.cuda.synchronize()
    _, _, n_ints = hip().chain_layout()
    cnt = torch.zeros(n_ints, dtype=torch.int32, device="cuda")
    h = torch.full((B, F), 3.0, dtype=torch.float16, device="cuda")
    out = resid.clone()
    hip().bmm_ffn_chain(tg.data_ptr(), int(Q4), F, K, dxh.data_ptr(), dxf.data_ptr(), nw.data_ptr(), 1e-5,
                        tdw.data_ptr(), int(td), h.data_ptr(), out.data_ptr(), B, cnt.data_ptr(), stream(), tr=tr)
    torch.cuda.synchronize()
    assert torch.equal(h, h_ref)
    r0 = resid.cpu().numpy()
    assert rel_err(out.cpu().numpy() - r0, out_ref.cpu().numpy() - r0) < 1e-5


@pytest.mark.parametrize("td", [Q4, Q6])
@pytest.mark.parametrize("B", [5, 6])
@pytest.mark.parametrize("tr", [0, 1])
def test_bmm_wo_ffn_chain_both_orientations(torch, td, B, tr):
    """bmm_wo_ffn_chain (Wo -> gate/up -> down in one launch) with its Wo and down roles in either
    orientation against the three separate launches (Wo and down at tr = 0), at
    test_bmm_wo_ffn_chain_matches_three_launches' tolerances."""
    F, K = CH_F, CH_K
    to_, _ = _tile16(Q4, K, K, 500, False, False)
    tg, _ = _tile16(Q4, 2 * F, K, 501, True, False)
    tdw, _ = _tile16(td, K, F, 502 + int(td), False, False)
    rng = np.random.default_rng(B * 7 + int(td))
    XA = rng.standard_normal((B, K)).astype(np.float32)
    dxa = torch.from_numpy(_swizzle4(XA.astype(np.float16))).cuda()
    resid0 = torch.from_numpy((rng.standard_normal((B, K)) * 2).astype(np.float32)).cuda()
    nw = torch.from_numpy((0.5 + rng.random(K)).astype(np.float32)).cuda()
    xh = torch.zeros(B, K, dtype=torch.float16, device="cuda")   # (unused: the norm path stages resid)
    r_ref = resid0.clone()
    h_ref = torch.zeros(B, F, dtype=torch.float16, device="cuda")
    hip().bmm(to_.data_ptr(), int(Q4), K, K, dxa.data_ptr(), K, r_ref.data_ptr(), K, B, stream(), tr=0)
    hip().bmm(tg.data_ptr(), int(Q4), 2 * F, K, xh.data_ptr(), K, 0, 0, B, stream(),
              h_out=h_ref.data_ptr(), ldh_out=F, xf=r_ref.data_ptr(), ldxf=K, norm=nw.data_ptr(), eps=1e-5)
    hip().bmm(tdw.data_ptr(), int(td), K, F, h_ref.data_ptr(), F, r_ref.data_ptr(), K, B, stream(), tr=0)
    torch.cuda.synchronize()
    _, _, n_ints = hip().chain_layout()
    cnt = torch.zeros(n_ints, dtype=torch.int32, device="cuda")
    r = resid0.clone()
    h = torch.full((B, F), 3.0, dtype=torch.float16, device="cuda")
    hip().bmm_wo_ffn_chain(to_.data_ptr(), int(Q4), K, dxa.data_ptr(), tg.data_ptr(), int(Q4), F, K, nw.data_ptr(), 1e-5,
                           tdw.data_ptr(), int(td), xh.data_ptr(), h.data_ptr(), r.data_ptr(), B, cnt.data_ptr(),
                           stream(), tr=tr)
    torch.cuda.synchronize()
    # the SwiGLU rows: equal up to the f16 rounding of inputs whose split-K sums differ in order
    hd = (h.float() - h_ref.float()).abs().max().item()
    assert hd <= 2e-2 * max(1.0, h_ref.float().abs().max().item()), hd
    r0 = resid0.cpu().numpy()
    assert rel_err(r.cpu().numpy() - r0, r_ref.cpu().numpy() - r0) < 1e-3
