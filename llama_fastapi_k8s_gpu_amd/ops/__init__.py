"""Torch-facing wrappers of the gfx950 HIP kernels (``csrc/kernels``).

These are the kernels the C++ engine schedules, exposed on ``torch`` tensors for
tests, experiments and custom pipelines. Every wrapper validates shapes, dtypes,
devices and contiguity on the host BEFORE the launch (a mis-shaped operand would
otherwise be an out-of-bounds access on the GPU) and runs on the current torch
stream. There is no fallback: without the ``_hip`` extension they raise.

    W = QuantMatrix.from_ggml(raw_bytes, GGMLType.Q4_K, rows, K)    # planar repack + upload
    y = gemv(W, x)                                  # y[rows] = W . x   (q8 activations, v_dot4)
    y = gemv(W, x, norm=w_norm)                     # RMSNorm fused into the prologue
    gemv(W, x, out=resid, accumulate=True)          # resid += W . x
    h = gemv_swiglu(W_gu, x, norm=w)                # silu(gate) * up, gate/up interleaved by 32 rows
    Y = gemm(W, X_bf16)                             # [T, rows] on MFMA with LDS-dequantised tiles
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

EPI_STORE, EPI_ADD, EPI_SWIGLU = 0, 1, 2
GEMM_STORE, GEMM_ADD, GEMM_SWIGLU = 0, 1, 2


def _hip():
    from ..runtime import load_hip
    return load_hip()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _check(t, dtype, shape=None, name="tensor"):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name} must be a CUDA (HIP) tensor")
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    return t.data_ptr()


@dataclass
class QuantMatrix:
    """A [rows, K] ggml-quantised matrix in the planar device layout."""
    data: "object"        # torch.uint8 CUDA tensor
    qtype: int
    rows: int
    K: int
    expert_stride: int = 0

    @classmethod
    def from_ggml(cls, raw: np.ndarray, qtype: int, rows: int, K: int, interleave_gate_up: bool = False,
                  raw_up: Optional[np.ndarray] = None) -> "QuantMatrix":
        import torch
        hip = _hip()
        raw = np.ascontiguousarray(np.frombuffer(raw, np.uint8) if isinstance(raw, (bytes, bytearray)) else raw)
        if raw.nbytes != hip.qbytes(int(qtype), rows, K):
            raise ValueError("raw block bytes do not match (type, rows, K)")
        if not interleave_gate_up:
            planar = hip.repack(int(qtype), raw, K, 0, rows, 0, K, rows, 0, 0)
            return cls(torch.from_numpy(planar).cuda(), int(qtype), rows, K)
        if raw_up is None:
            raise ValueError("interleave_gate_up needs raw_up")
        g = hip.repack(int(qtype), raw, K, 0, rows, 0, K, 2 * rows, 32, 0)
        u = hip.repack(int(qtype), np.ascontiguousarray(raw_up), K, 0, rows, 0, K, 2 * rows, 32, 32)
        return cls(torch.from_numpy(g | u).cuda(), int(qtype), 2 * rows, K)


def _x_ptr(x, K, norm):
    import torch
    xp = _check(x, torch.float32, (K,), "x")
    if K % 256 and K % 32:
        raise ValueError("K must be a multiple of 32")
    np_ = _check(norm, torch.float32, (K,), "norm") if norm is not None else 0
    return xp, np_


def gemv(W: QuantMatrix, x, norm=None, eps: float = 1e-5, out=None, accumulate: bool = False):
    """y = W . x  (optionally x <- rmsnorm(x) * norm; optionally out += W . x)."""
    import torch
    xp, npp = _x_ptr(x, W.K, norm)
    if out is None:
        if accumulate:
            raise ValueError("accumulate needs out")
        out = torch.empty(W.rows, device=x.device, dtype=torch.float32)
    op = _check(out, torch.float32, (W.rows,), "out")
    _hip().gemv(W.data.data_ptr(), W.qtype, W.rows, W.K, xp, npp, eps, op, W.rows,
                EPI_ADD if accumulate else EPI_STORE, _stream())
    return out


def gemv_swiglu(W_gu: QuantMatrix, x, norm=None, eps: float = 1e-5):
    """silu(gate . x) * (up . x) for a gate/up matrix interleaved in 32-row groups."""
    import torch
    if W_gu.rows % 64:
        raise ValueError("gate/up matrix must have a multiple of 64 rows")
    xp, npp = _x_ptr(x, W_gu.K, norm)
    F = W_gu.rows // 2
    out = torch.empty(F, device=x.device, dtype=torch.float32)
    _hip().gemv(W_gu.data.data_ptr(), W_gu.qtype, W_gu.rows, W_gu.K, xp, npp, eps, out.data_ptr(), F, EPI_SWIGLU,
                _stream())
    return out


def gemm(W: QuantMatrix, x_bf16, out=None, accumulate: bool = False):
    """Y[T, rows] = X[T, K] . W^T on MFMA (weights dequantised into LDS tiles)."""
    import torch
    if x_bf16.dim() != 2 or x_bf16.shape[1] != W.K:
        raise ValueError(f"x must be [T, {W.K}]")
    T = int(x_bf16.shape[0])
    xp = _check(x_bf16, torch.bfloat16, None, "x")
    if out is None:
        if accumulate:
            raise ValueError("accumulate needs out")
        out = torch.empty(T, W.rows, device=x_bf16.device, dtype=torch.float32)
    op = _check(out, torch.float32, (T, W.rows), "out")
    _hip().gemm(W.data.data_ptr(), W.qtype, W.rows, W.K, xp, T, op, 0, W.rows,
                GEMM_ADD if accumulate else GEMM_STORE, _stream())
    return out


def rmsnorm_bf16(x, w, eps: float = 1e-5):
    import torch
    if x.dim() != 2:
        raise ValueError("x must be [T, d]")
    T, d = map(int, x.shape)
    xp = _check(x, torch.float32, (T, d), "x")
    wp = _check(w, torch.float32, (d,), "w")
    y = torch.empty(T, d, device=x.device, dtype=torch.bfloat16)
    _hip().rmsnorm_bf16(xp, wp, eps, T, d, y.data_ptr(), _stream())
    return y


def embed(W: QuantMatrix, tokens):
    """Dequantised rows W[tokens] -> float32 [T, K]."""
    import torch
    tp = _check(tokens, torch.int32, None, "tokens")
    T = int(tokens.numel())
    if T and (int(tokens.min()) < 0 or int(tokens.max()) >= W.rows):
        raise ValueError("token id out of range")
    out = torch.empty(T, W.K, device=tokens.device, dtype=torch.float32)
    _hip().embed(W.data.data_ptr(), W.qtype, W.rows, W.K, tp, T, out.data_ptr(), _stream())
    return out


def attention_decode(q, k_cache, v_cache, pos: int, scale: Optional[float] = None, live: int = 0):
    """One query token per head against keys [0, pos] of an f16 cache [n_kv, n_ctx, hd].

    live: which keys a block loads (AttnDecodeArgs::live) - 0 all 64 of every launched split, 1 only
    those below the length, 2 those spread evenly over the launched splits."""
    import torch
    n_kv, n_ctx, hd = map(int, k_cache.shape)
    n_head = int(q.numel()) // hd
    if n_head % n_kv or not 0 <= pos < n_ctx or hd not in (64, 128):
        raise ValueError("bad attention shapes")
    qp = _check(q, torch.float32, (n_head * hd,), "q")
    kp = _check(k_cache, torch.float16, (n_kv, n_ctx, hd), "k_cache")
    vp = _check(v_cache, torch.float16, (n_kv, n_ctx, hd), "v_cache")
    hip = _hip()
    part = torch.empty(hip.attn_decode_workspace_floats(n_ctx, n_head, hd), device=q.device, dtype=torch.float32)
    cnt = torch.zeros(64, device=q.device, dtype=torch.int32)
    p = torch.tensor([pos], device=q.device, dtype=torch.int32)
    out = torch.empty(n_head * hd, device=q.device, dtype=torch.float32)
    hip.attn_decode(qp, kp, vp, p.data_ptr(), n_ctx, n_head, n_kv, hd, scale or hd ** -0.5, part.data_ptr(),
                    out.data_ptr(), _stream(), cnt.data_ptr(), live=live)
    return out


def attention_prefill(q, k_cache, v_cache, pos0: int, scale: Optional[float] = None):
    """Causal attention of T query tokens (positions pos0..pos0+T-1) -> [T, n_head*hd]."""
    import torch
    n_kv, n_ctx, hd = map(int, k_cache.shape)
    T = int(q.shape[0])
    n_head = int(q.shape[1]) // hd
    if n_head % n_kv or pos0 < 0 or pos0 + T > n_ctx or hd not in (64, 128):
        raise ValueError("bad attention shapes")
    qp = _check(q, torch.float32, (T, n_head * hd), "q")
    kp = _check(k_cache, torch.float16, (n_kv, n_ctx, hd), "k_cache")
    vp = _check(v_cache, torch.float16, (n_kv, n_ctx, hd), "v_cache")
    out = torch.empty(T, n_head * hd, device=q.device, dtype=torch.float32)
    _hip().attn_prefill(qp, kp, vp, T, pos0, n_ctx, n_head, n_kv, hd, scale or hd ** -0.5, out.data_ptr(),
                        _stream())
    return out


def _ws(nbytes, device):
    import torch
    return torch.zeros((nbytes + 3) // 4, device=device, dtype=torch.int32)


def moe_router_wide(x, norm, W, k: int, eps: float = 1e-5):
    """Rows x [B, d] -> RMSNorm * norm -> F32 router W [E, d] (17 <= E <= 256) -> softmax, top-k (lowest
    id on a tie), renormalised. Returns (ids [B, k] int32, weights [B, k], logits [B, E])."""
    import torch
    B, d = map(int, x.shape)
    E = int(W.shape[0])
    hip = _hip()
    if not hip.moe_router_wide_ok(0, E, k, d):
        raise ValueError("moe_router_wide: 17 <= E <= 256, k <= 16, d a multiple of 4 up to 15360")
    xp, npp, wp = _check(x, torch.float32, (B, d), "x"), _check(norm, torch.float32, (d,), "norm"), \
        _check(W, torch.float32, (E, d), "W")
    ids = torch.empty(B, k, device=x.device, dtype=torch.int32)
    w = torch.empty(B, k, device=x.device, dtype=torch.float32)
    logits = torch.empty(B, E, device=x.device, dtype=torch.float32)
    ws = _ws(hip.moe_router_wide_workspace(B, E), x.device)
    hip.moe_router_wide(xp, d, B, npp, eps, wp, d, E, k, ws.data_ptr(), logits.data_ptr(), ids.data_ptr(), w.data_ptr(),
                        _stream())
    return ids, w, logits


def moe_route_group_wide(E: int, k: int, logits=None, sel=None, selw=None):
    """Per-expert row lists (ascending token order) and the grouped GEMM's work list, from router
    logits [T, E] or from picks sel / selw [T, k]. Returns a dict of sel, selw, cnt_off [E + 1], tok,
    gw, pos [T k], items [bound, 3] = (expert, first row, rows), n_items [1]."""
    import torch
    hip = _hip()
    if (logits is None) == (sel is None) or not 1 <= k <= min(16, E) or E > 256:
        raise ValueError("moe_route_group_wide: logits or sel / selw; E <= 256, k <= 16")
    if logits is not None:
        T, dev = int(logits.shape[0]), logits.device
        lp = _check(logits, torch.float32, (T, E), "logits")
        sel = torch.empty(T, k, device=dev, dtype=torch.int32)
        selw = torch.empty(T, k, device=dev, dtype=torch.float32)
    else:
        T, dev, lp = int(sel.shape[0]), sel.device, 0
        if int(sel.min()) < 0 or int(sel.max()) >= E:
            raise ValueError("expert id out of range")
    sp, swp = _check(sel, torch.int32, (T, k), "sel"), _check(selw, torch.float32, (T, k), "selw")
    i32 = lambda n: torch.empty(n, device=dev, dtype=torch.int32)
    o = dict(sel=sel, selw=selw, cnt_off=i32(E + 1), tok=i32(T * k), gw=torch.empty(T * k, device=dev), pos=i32(T * k),
             items=torch.empty(hip.moe_group_wide_items(T, E, k), 3, device=dev, dtype=torch.int32), n_items=i32(1))
    ws = _ws(hip.moe_group_wide_workspace(T, E), dev)
    hip.moe_route_group_wide(lp, T, E, k, sp, swp, o["cnt_off"].data_ptr(), o["tok"].data_ptr(), o["gw"].data_ptr(),
                             o["pos"].data_ptr(), o["items"].data_ptr(), o["n_items"].data_ptr(), ws.data_ptr(), _stream())
    return o


def moe_gemm_grouped(w_t16, qtype: int, d: int, F: int, E: int, x, routing, swiglu: bool):
    """One projection of every routed expert in one launch over ``routing`` (moe_route_group_wide's dict).
    swiglu: w_t16 = the experts' SwiGLU tile16 copies back to back, x f16 [T k, d] -> f16 [T k, F];
    else: w_t16 = the down experts concatenated along K, x f16 [T k, F] -> f32 [T k, d]. Rows in gathered
    order, f16 in the batched kernels' 4-group k order."""
    import torch
    hip = _hip()
    R, Kin, n_out = int(routing["tok"].numel()), (d if swiglu else F), (F if swiglu else d)
    xp = _check(x, torch.float16, (R, Kin), "x")
    rows = 2 * F if swiglu else d
    if not hip.moe_gemm_grouped_ok(int(qtype), rows, Kin):
        raise ValueError("moe_gemm_grouped: a tile16 weight type, K a multiple of 256, rows a multiple of 16")
    need = E * hip.t16_bytes(int(qtype), rows, Kin)
    if _check(w_t16, torch.uint8, None, "w_t16") == 0 or w_t16.numel() != need:
        raise ValueError(f"w_t16 must hold {need} bytes")
    out = torch.empty(R, n_out, device=x.device, dtype=torch.float16 if swiglu else torch.float32)
    hip.moe_gemm_grouped(w_t16.data_ptr(), int(qtype), d, F, E, xp, out.data_ptr(), bool(swiglu),
                         routing["items"].data_ptr(), routing["n_items"].data_ptr(), int(routing["items"].shape[0]),
                         _stream())
    return out


__all__ = ["QuantMatrix", "gemv", "gemv_swiglu", "gemm", "rmsnorm_bf16", "embed", "attention_decode",
           "attention_prefill", "moe_router_wide", "moe_route_group_wide", "moe_gemm_grouped"]
