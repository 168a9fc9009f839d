"""The BF16 kernels against fp64 over their own operands (the bf16 weight values exactly, x as the
kernel receives it): the decode GEMV family with f32 activations, gemm_bf16w (gemm_w16.hip, reached
through gemm_dq) in both token regimes, and the embedding gather.

Bounds are derived, not measured. fp32 accumulation of exact products in any order (split-K atomics
included) stays within B = 2 K 2^-24 sum_k |W_jk x_k| of fp64 (tests/test_score_head_gpu.py's form);
K >= 64 leaves room in it for the one f32 rounding of x * w_norm and the 1/rms factor. On top: 2^-24
|y| per further f32 operation on y (residual add, rotation); the SwiGLU s(g) u with |s'| <= 1.1
propagates 1.1 |u| B_g + |s(g)| B_u, its exp / divide / multiplies are given 32 ulp (|g| < 8 here),
and gemm's bf16 output one 2^-8 rounding; gemm's resid / ADD value p is rounded once per K part
(at most 4 here) as the atomics pass it: 4 * 2^-24 |p|; K / V cache rows one f16 rounding (2^-11). A run
rewrites profiles/bf16_test_figures.txt with each case's worst error / bound ratio."""
import os

import numpy as np
import pytest

from llama_fastapi_k8s_gpu_amd.gguf.constants import GGMLType
from llama_fastapi_k8s_gpu_amd.gguf.quants import dequantize, quantize
from llama_fastapi_k8s_gpu_amd.ops import EPI_STORE, EPI_SWIGLU, GEMM_ADD, GEMM_STORE, GEMM_SWIGLU
from gpu_helpers import hip, stream

pytestmark = pytest.mark.gpu
BF16, U, EPS = int(GGMLType.BF16), 2.0 ** -24, 1e-5
FIGURES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bf16_test_figures.txt")


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _weights(torch, R, K, seed):
    """(device bytes, fp64 [R][K]) of a bf16 matrix; the planar layout of BF16 is the GGUF's own."""
    raw = quantize((np.random.default_rng(seed).standard_normal(R * K) * 0.05).astype(np.float32), GGMLType.BF16)
    return torch.from_numpy(raw).cuda(), dequantize(raw, GGMLType.BF16, R * K).reshape(R, K).astype(np.float64)


def _ref(W, x):
    """fp64 W x and the accumulation bound B, for x [K] or [T][K] (-> [T][R])."""
    return x @ W.T, 2 * W.shape[1] * U * (np.abs(x) @ np.abs(W).T)


def _silu(g):
    return g / (1 + np.exp(-g))


_figures = {}   # tag -> worst ratio of this run; the file is rewritten whole, one line per case


def _report(tag, got, ref, bound):
    ratio = float(np.max(np.abs(got - ref) / bound))
    _figures[tag] = max(ratio, _figures.get(tag, 0.0))
    os.makedirs(os.path.dirname(FIGURES), exist_ok=True)
    with open(FIGURES, "w") as f:
        f.writelines(f"{t}: worst |error| / bound = {r:.3g}\n" for t, r in sorted(_figures.items()))
    assert np.isfinite(got).all() and ratio <= 1.0, (tag, ratio)


@pytest.mark.parametrize("launch", ["plain", "resid", "swiglu", "qkv"])
@pytest.mark.parametrize("rows", [32, 1000])
@pytest.mark.parametrize("K", [256, 4096])
def test_gemv_bf16(torch, K, rows, launch):
    rng = np.random.default_rng(K + rows)
    x, nw = rng.standard_normal(K).astype(np.float32), (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    dx, dn = torch.from_numpy(x).cuda(), torch.from_numpy(nw).cuda()
    xn = x.astype(np.float64) * nw / np.sqrt(np.mean(x.astype(np.float64) ** 2) + EPS)   # what the norm launches multiply
    tag = f"gemv {launch} K={K} rows={rows}"
    if launch in ("plain", "resid"):
        dw, W = _weights(torch, rows, K, 1)
        res = rng.standard_normal(rows).astype(np.float32)
        dres = torch.from_numpy(res).cuda()
        out = torch.full((rows + 8,), float("nan"), device="cuda")
        hip().gemv(dw.data_ptr(), BF16, rows, K, dx.data_ptr(), 0, EPS, out.data_ptr(), rows, EPI_STORE, stream(),
                   resid=dres.data_ptr() if launch == "resid" else 0)
        ref, B = _ref(W, x.astype(np.float64))
        if launch == "resid":
            ref, B = ref + res, B + U * np.abs(ref + res)
        got = out.cpu().numpy()
        assert np.isnan(got[rows:]).all(), tag
        _report(tag, got[:rows], ref, B)
    elif launch == "swiglu":   # features: rows up to a multiple of 32; gate/up interleaved in 32-row groups
        F = -(-rows // 32) * 32
        dw, W = _weights(torch, 2 * F, K, 2)
        out = torch.full((F + 8,), float("nan"), device="cuda")
        hip().gemv(dw.data_ptr(), BF16, 2 * F, K, dx.data_ptr(), dn.data_ptr(), EPS, out.data_ptr(), F, EPI_SWIGLU, stream())
        y, B = _ref(W, xn)
        (g, u), (Bg, Bu) = (v.reshape(-1, 2, 32).transpose(1, 0, 2).reshape(2, F) for v in (y, B))
        got = out.cpu().numpy()
        assert np.isnan(got[F:]).all(), tag
        _report(tag, got[:F], _silu(g) * u, 1.1 * np.abs(u) * Bg + np.abs(_silu(g)) * Bu + 32 * U * np.abs(_silu(g) * u))
    else:   # Q|K|V + RoPE + f16 KV append at position 5 of 9, sentinel caches
        hd, nkv, n_ctx, pos = 8, 24, 9, 5
        (dq, Wq), (dk, Wk), (dv, Wv) = (_weights(torch, r, K, 3 + i) for i, r in enumerate((rows, nkv, nkv)))
        ang = rng.uniform(0, 6.28, (n_ctx, hd // 2))
        rope = np.stack([np.cos(ang), np.sin(ang)], -1).astype(np.float32)
        q_out = torch.full((rows + 8,), float("nan"), device="cuda")
        kc, vc = (torch.full((nkv // hd, n_ctx, hd), 777.0, dtype=torch.float16, device="cuda") for _ in range(2))
        dpos, drope = torch.tensor([pos], dtype=torch.int32, device="cuda"), torch.from_numpy(rope).cuda()
        hip().gemv_qkv(dq.data_ptr(), BF16, dk.data_ptr(), BF16, dv.data_ptr(), BF16, rows, nkv, K, dx.data_ptr(),
                       dn.data_ptr(), EPS, q_out.data_ptr(), kc.data_ptr(), vc.data_ptr(), n_ctx, hd, dpos.data_ptr(),
                       drope.data_ptr(), stream())

        def rot(y, B):   # pairs (2j, 2j+1) of every head by (cos, sin)[pos][j]
            c, s = (np.tile(rope[pos, :, i].astype(np.float64), y.size // hd) for i in (0, 1))
            e, o, Be, Bo = y[0::2], y[1::2], B[0::2], B[1::2]
            r = np.stack([e * c - o * s, e * s + o * c], -1).reshape(-1)
            return r, np.stack([np.abs(c) * Be + np.abs(s) * Bo] * 2, -1).reshape(-1) + 4 * U * np.abs(r).max()
        got = q_out.cpu().numpy()
        assert np.isnan(got[rows:]).all(), tag
        _report(tag + " q", got[:rows], *rot(*_ref(Wq, xn)))
        for name, cache, (r, B) in (("k", kc, rot(*_ref(Wk, xn))), ("v", vc, _ref(Wv, xn))):
            c = cache.cpu().numpy().astype(np.float64)
            assert (np.delete(c, pos, axis=1) == 777.0).all(), (tag, name, "a row other than pos changed")
            _report(f"{tag} {name}", c[:, pos].reshape(-1), r, B + 2.0 ** -11 * np.abs(r) + 2.0 ** -24)


@pytest.mark.parametrize("N", [64, 160, 256])
@pytest.mark.parametrize("K", [64, 192, 1024])
@pytest.mark.parametrize("T", [1, 6, 16, 17, 64, 65, 130])
def test_gemm_bf16w(torch, T, K, N):
    """STORE, STORE + resid, ADD onto a prefilled buffer and (N % 64 == 0) SWIGLU; `out` inside a NaN
    buffer with a guard row and guard columns, X with a NaN row behind row T - 1; every case twice."""
    rng = np.random.default_rng(T * 7 + K + N)
    dw, W = _weights(torch, N, K, N + K)
    xb = torch.from_numpy(rng.standard_normal((T + 1, K)).astype(np.float32)).cuda().to(torch.bfloat16)
    xb[T] = float("nan")
    x = xb[:T].float().cpu().numpy().astype(np.float64)
    ref, B = _ref(W, x)
    pre = rng.standard_normal((T, N)).astype(np.float32)
    ldo = N + 8
    dpre = torch.from_numpy(pre).cuda()
    dres = torch.zeros(T, ldo, device="cuda")   # resid has out's row stride
    dres[:, :N] = dpre
    split = K == 1024   # 16 K steps: both regimes split a grid this small (launch_bf16w)
    for epi in ["store", "resid", "add"] + (["swiglu"] if N % 64 == 0 else []):
        runs = []
        for _ in range(2):
            if epi == "swiglu":
                out = torch.full((T + 1, N // 2), float("nan"), dtype=torch.bfloat16, device="cuda")
                hip().gemm(dw.data_ptr(), BF16, N, K, xb.data_ptr(), T, 0, out.data_ptr(), 0, GEMM_SWIGLU, stream(), 0, 0, 0, False)
                got, guard = out[:T].float().cpu().numpy(), out[T:].float().cpu().numpy()
            else:
                out = torch.full((T + 1, ldo), float("nan"), device="cuda")
                if epi == "add":
                    out[:T, :N] = dpre
                hip().gemm(dw.data_ptr(), BF16, N, K, xb.data_ptr(), T, out.data_ptr(), 0, ldo, GEMM_ADD if epi == "add" else GEMM_STORE,
                           stream(), dres.data_ptr() if epi == "resid" else 0, 0, 0, False)
                o = out.cpu().numpy()
                got, guard = o[:T, :N], np.concatenate([o[T], o[:T, N:].reshape(-1)])
            assert np.isnan(guard).all(), (epi, T, K, N, "guard overwritten")
            runs.append(got)
        if epi == "swiglu":
            (g, u), (Bg, Bu) = (v.reshape(T, -1, 2, 32).transpose(2, 0, 1, 3).reshape(2, T, N // 2) for v in (ref, B))
            r = _silu(g) * u
            bound = 1.1 * np.abs(u) * Bg + np.abs(_silu(g)) * Bu + (32 * U + 2.0 ** -8) * np.abs(r)
        else:
            r = ref if epi == "store" else ref + pre
            bound = B + (0 if epi == "store" else U * np.abs(r) + 4 * U * np.abs(pre))
        if epi == "store" and not split:
            assert (runs[0].view(np.uint32) == runs[1].view(np.uint32)).all(), (T, K, N, "not reproducible")
        for got in runs:
            _report(f"gemm {epi} T={T} K={K} N={N}", got, r, bound)


def test_embed_rows_bf16(torch):
    V, d = 50, 96
    dw, W = _weights(torch, V, d, 9)
    ids = torch.tensor([0, V - 1, 17], dtype=torch.int32, device="cuda")
    out = torch.full((3, d), float("nan"), device="cuda")
    hip().embed(dw.data_ptr(), BF16, V, d, ids.data_ptr(), 3, out.data_ptr(), stream())
    assert (out.cpu().numpy().astype(np.float64) == W[[0, V - 1, 17]]).all()
