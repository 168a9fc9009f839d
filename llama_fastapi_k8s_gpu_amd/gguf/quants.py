"""NumPy reference implementation of the ggml block formats used by Q4_K_M /
Q8_0 and the legacy Q4_0 / Q4_1 / Q5_0 / Q5_1 GGUF files: Q4_K, Q5_K, Q6_K, Q8_0,
Q4_0, Q4_1, Q5_0, Q5_1, the 2- and 3-bit K-quants Q2_K, Q3_K, and the non-linear 4-bit pair
IQ4_NL, IQ4_XS (+ F16/BF16/F32).

This is the *reference* every native path is tested against (T1 in SURVEY
§4.3): the C++ CPU backend, the GPU repack and the HIP kernels must reproduce
``dequantize`` exactly (up to f32 rounding).

Block layouts:
  Q8_0  34 B / 32 w : d f16 | qs int8[32]                 w = d*q
  Q4_0  18 B / 32 w : d f16 | qs[16]                      w = d*(q-8)
  Q4_1  20 B / 32 w : d f16 | m f16 | qs[16]              w = d*q + m
  Q5_0  22 B / 32 w : d f16 | qh u32 | qs[16]             w = d*(q-16)   (5th bit from qh)
  Q5_1  24 B / 32 w : d f16 | m f16 | qh u32 | qs[16]     w = d*q + m
                      (weight j < 16: low nibble of qs[j], bit j of qh;
                       weight j + 16: high nibble of qs[j], bit j + 16 of qh)
  Q4_K 144 B / 256 w: d f16 | dmin f16 | scales[12] | qs[128]
                      w = d*sc_j*q - dmin*m_j ; 6-bit (sc,m) packed, get_scale_min_k4
  Q5_K 176 B / 256 w: d | dmin | scales[12] | qh[32] | qs[128]  (5th bit from qh)
  Q6_K 210 B / 256 w: ql[128] | qh[64] | scales int8[16] | d f16  w = d*sc*(q-32)
  Q2_K  84 B / 256 w: scales[16] | qs[64] | d f16 | dmin f16
                      weight i: n = i//128, j = (i%128)//32, l = i%32, sub-block s = i//16
                      q = (qs[32n+l] >> 2j) & 3 ; w = d*(scales[s]&0xF)*q - dmin*(scales[s]>>4)
  Q3_K 110 B / 256 w: hmask[32] | qs[64] | scales[12] | d f16
                      q = ((qs[32n+l] >> 2j) & 3) + 4*((hmask[l] >> (4n+j)) & 1) - 4
                      sc[s] = 6 bits: low nibble scales[s]&0xF (s<8) / scales[s-8]>>4,
                      top two bits (scales[8+s%4] >> 2*(s//4)) & 3 ; w = d*(sc[s]-32)*q
  IQ4_NL 18 B / 32 w: d f16 | qs[16]   w[j] = d*KVALUES_IQ4[qs[j]&15], w[j+16] = d*KVALUES_IQ4[qs[j]>>4]
  IQ4_XS 136 B / 256 w: d f16 | scales_h u16 | scales_l[4] | qs[128]
                      sub-block ib = 0..7 (weights 32ib..32ib+31, bytes qs[16ib..16ib+15], nibble
                      order as IQ4_NL): ls = ((scales_l[ib//2] >> 4*(ib%2)) & 15) |
                      (((scales_h >> 2*ib) & 3) << 4) ; w = d*(ls-32)*KVALUES_IQ4[nibble]

The quantisers are simple (min/max per sub-block, no iterative search) - they
produce valid blocks with bounded error, which is all the synthetic-model and
test paths need; decoding is what must match real llama.cpp files.
"""
from __future__ import annotations

import numpy as np

from .constants import GGML_BLOCK, QK_K, GGMLType

# ----------------------------------------------------------------- helpers


def _f16(a) -> np.ndarray:
    return np.asarray(a, dtype=np.float32).astype(np.float16)


def _unpack_scale_min_k4(scales: np.ndarray):
    """scales: uint8 [nb, 12] -> (sc, m) uint8 [nb, 8] (ggml get_scale_min_k4)."""
    s = scales.astype(np.uint8)
    sc = np.empty((s.shape[0], 8), np.uint8)
    m = np.empty((s.shape[0], 8), np.uint8)
    sc[:, :4] = s[:, 0:4] & 63
    m[:, :4] = s[:, 4:8] & 63
    sc[:, 4:] = (s[:, 8:12] & 0xF) | ((s[:, 0:4] >> 6) << 4)
    m[:, 4:] = (s[:, 8:12] >> 4) | ((s[:, 4:8] >> 6) << 4)
    return sc, m


def _pack_scale_min_k4(sc: np.ndarray, m: np.ndarray) -> np.ndarray:
    """Inverse of _unpack_scale_min_k4; sc, m uint8 [nb, 8] with values < 64."""
    sc = sc.astype(np.uint8)
    m = m.astype(np.uint8)
    out = np.zeros((sc.shape[0], 12), np.uint8)
    out[:, 0:4] = (sc[:, 0:4] & 63) | ((sc[:, 4:8] >> 4) << 6)
    out[:, 4:8] = (m[:, 0:4] & 63) | ((m[:, 4:8] >> 4) << 6)
    out[:, 8:12] = (sc[:, 4:8] & 0xF) | ((m[:, 4:8] & 0xF) << 4)
    return out


def _blocks(data: np.ndarray, ggml_type) -> np.ndarray:
    bs, bb = GGML_BLOCK[GGMLType(ggml_type)]
    raw = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray)
                               else data.view(np.uint8).reshape(-1))
    assert raw.size % bb == 0
    return raw.reshape(-1, bb)



LEGACY_TYPES = (GGMLType.Q4_0, GGMLType.Q4_1, GGMLType.Q5_0, GGMLType.Q5_1)


def _legacy_fields(b: np.ndarray, t):
    """Blocks uint8 [nb, bytes] of a legacy type -> (d f16 [nb], m f16 [nb] or None, q uint8 [nb, 32])."""
    has_m = t in (GGMLType.Q4_1, GGMLType.Q5_1)
    has_h = t in (GGMLType.Q5_0, GGMLType.Q5_1)
    o = 0
    d = b[:, 0:2].copy().view(np.float16)[:, 0]
    o += 2
    m = None
    if has_m:
        m = b[:, o:o + 2].copy().view(np.float16)[:, 0]
        o += 2
    qh = None
    if has_h:
        qh = b[:, o:o + 4].copy().view("<u4")[:, 0]
        o += 4
    qs = b[:, o:o + 16]
    q = np.concatenate([qs & 0xF, qs >> 4], axis=1).astype(np.uint8)
    if has_h:
        bits = ((qh[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1).astype(np.uint8)
        q |= bits << 4
    return d, m, q


def _legacy_offset(t) -> int:
    return 8 if t == GGMLType.Q4_0 else 16


K23_TYPES = (GGMLType.Q2_K, GGMLType.Q3_K)

IQ4_TYPES = (GGMLType.IQ4_NL, GGMLType.IQ4_XS)

# the 16-entry codebook a nibble of IQ4_NL / IQ4_XS indexes
KVALUES_IQ4 = np.array([-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113], np.int8)


def _iq4_fields(b: np.ndarray, t):
    """Blocks uint8 [nb, bytes] of IQ4_NL / IQ4_XS -> (kv int16 [nb, bs] codebook values in weight
    order, l int16 [nb, bs // 32] sub-block multipliers (ls - 32; 1 for IQ4_NL), d f16 [nb]):
    w = d * l[i // 32] * kv[i]."""
    d = b[:, 0:2].copy().view(np.float16)[:, 0]
    if t == GGMLType.IQ4_NL:
        qs = b[:, 2:18].reshape(-1, 1, 16)
        l = np.ones((b.shape[0], 1), np.int16)
    else:
        sh = b[:, 2:4].copy().view("<u2")[:, 0].astype(np.uint32)
        sl = b[:, 4:8]
        ib = np.arange(8)
        low = (sl[:, ib // 2] >> (4 * (ib % 2)).astype(np.uint8)) & 15
        top = (sh[:, None] >> (2 * ib).astype(np.uint32)[None, :]) & 3
        l = (low.astype(np.int16) | (top.astype(np.int16) << 4)) - 32
        qs = b[:, 8:136].reshape(-1, 8, 16)
    idx = np.concatenate([qs & 0xF, qs >> 4], axis=2)  # [nb, sub-blocks, 32]
    kv = KVALUES_IQ4[idx].astype(np.int16).reshape(b.shape[0], -1)
    return kv, l, d


def _iq4_nearest(r: np.ndarray) -> np.ndarray:
    """Index of the codebook entry nearest to each element of r."""
    return np.abs(r[..., None] - KVALUES_IQ4.astype(np.float64)).argmin(axis=-1).astype(np.uint8)


def _unpack_q3k_scales(scales: np.ndarray) -> np.ndarray:
    """scales: uint8 [nb, 12] -> the sixteen 6-bit scales, uint8 [nb, 16] (0..63, before the -32)."""
    s = scales.astype(np.uint8)
    low = np.concatenate([s[:, 0:8] & 0xF, s[:, 0:8] >> 4], axis=1)
    idx = np.arange(16)
    top = (s[:, 8 + idx % 4] >> (2 * (idx // 4)).astype(np.uint8)) & 3
    return (low | (top << 4)).astype(np.uint8)


def _pack_q3k_scales(sc: np.ndarray) -> np.ndarray:
    """Inverse of _unpack_q3k_scales; sc uint8 [nb, 16] with values < 64."""
    sc = sc.astype(np.uint8)
    out = np.zeros((sc.shape[0], 12), np.uint8)
    out[:, 0:8] = (sc[:, 0:8] & 0xF) | ((sc[:, 8:16] & 0xF) << 4)
    for s in range(16):
        out[:, 8 + s % 4] |= ((sc[:, s] >> 4) & 3) << (2 * (s // 4))
    return out


def _unpack_2bit(qs: np.ndarray) -> np.ndarray:
    """qs uint8 [nb, 64] -> the 2-bit fields in weight order, uint8 [nb, 256]."""
    out = np.empty((qs.shape[0], 256), np.uint8)
    for n in range(2):
        for j in range(4):
            out[:, 128 * n + 32 * j:128 * n + 32 * j + 32] = (qs[:, 32 * n:32 * n + 32] >> (2 * j)) & 3
    return out


def _pack_2bit(q: np.ndarray) -> np.ndarray:
    qs = np.zeros((q.shape[0], 64), np.uint8)
    for n in range(2):
        for j in range(4):
            qs[:, 32 * n:32 * n + 32] |= (q[:, 128 * n + 32 * j:128 * n + 32 * j + 32] & 3).astype(np.uint8) << (2 * j)
    return qs


def _k23_fields(b: np.ndarray, t):
    """Blocks uint8 [nb, bytes] of Q2_K / Q3_K -> (q int16 [nb, 256], sc int16 [nb, 16],
    m int16 [nb, 16] or None, d f16 [nb], dmin f16 [nb] or None): w = d*sc[i//16]*q - dmin*m[i//16]."""
    if t == GGMLType.Q2_K:
        scales = b[:, 0:16]
        q = _unpack_2bit(b[:, 16:80]).astype(np.int16)
        d = b[:, 80:82].copy().view(np.float16)[:, 0]
        dmin = b[:, 82:84].copy().view(np.float16)[:, 0]
        return q, (scales & 0xF).astype(np.int16), (scales >> 4).astype(np.int16), d, dmin
    hmask = b[:, 0:32]
    q = _unpack_2bit(b[:, 32:96]).astype(np.int16)
    for n in range(2):
        for j in range(4):
            q[:, 128 * n + 32 * j:128 * n + 32 * j + 32] += 4 * ((hmask >> (4 * n + j)) & 1).astype(np.int16)
    q -= 4
    sc = _unpack_q3k_scales(b[:, 96:108]).astype(np.int16) - 32
    d = b[:, 108:110].copy().view(np.float16)[:, 0]
    return q, sc, None, d, None

# ------------------------------------------------------------- dequantise


def dequantize(data, ggml_type, n_elements: int | None = None, arith: str = "f32") -> np.ndarray:
    """Decode raw ggml bytes into float32 (flat).

    ``arith="f16"`` reproduces the batched decode projection's dequantisation bit for bit
    (kernels/bmm.hip on its tile16 copy): the per-sub-block scale d*sc and offset -dmin*m are
    rounded to f16 once, and every weight is ONE f16 rounding of q*scale + offset (a fused
    v_pk_fma_f16). Q2_K: scale f16(d*(scales[s]&0xF)), offset f16(-dmin*(scales[s]>>4)), products
    taken in f32, q in 0..3. Q3_K: scale f16(d*(sc[s]-32)), no offset, q in -4..3 (the -4 is
    removed exactly before the multiply). IQ4_NL / IQ4_XS: scale d / f16(d*(ls-32)) (the product is
    exact in f32), no offset, and every weight is one f16 rounding of codebook value * scale.
    Returned as float32 (exact f16 values)."""
    t = GGMLType(ggml_type)
    if arith == "f16" and t in (GGMLType.Q8_0, GGMLType.Q4_K, GGMLType.Q5_K, GGMLType.Q6_K) + LEGACY_TYPES + K23_TYPES \
            + IQ4_TYPES:
        return _dequantize_f16(data, t, n_elements)
    if t == GGMLType.F32:
        return np.frombuffer(bytes(data) if not isinstance(data, np.ndarray) else data.tobytes(),
                             dtype=np.float32).copy()
    if t == GGMLType.F16:
        return np.asarray(data).view(np.uint8).reshape(-1).view(np.float16).astype(np.float32)
    if t == GGMLType.BF16:
        u = np.asarray(data).view(np.uint8).reshape(-1).view(np.uint16).astype(np.uint32) << 16
        return u.view(np.float32).copy()
    b = _blocks(data, t)
    nb = b.shape[0]
    if t == GGMLType.Q8_0:
        d = b[:, 0:2].copy().view(np.float16).astype(np.float32)  # [nb,1]
        q = b[:, 2:34].view(np.int8).astype(np.float32)
        out = d * q
    elif t in LEGACY_TYPES:
        d, m, q = _legacy_fields(b, t)
        d = d.astype(np.float32)[:, None]
        if m is None:
            out = d * (q.astype(np.float32) - np.float32(_legacy_offset(t)))
        else:
            out = d * q.astype(np.float32) + m.astype(np.float32)[:, None]
    elif t in K23_TYPES:
        q, sc, m, d, dmin = _k23_fields(b, t)
        a = np.repeat(d.astype(np.float32)[:, None] * sc.astype(np.float32), 16, axis=1)
        out = a * q.astype(np.float32)
        if m is not None:
            out -= np.repeat(dmin.astype(np.float32)[:, None] * m.astype(np.float32), 16, axis=1)
    elif t in IQ4_TYPES:
        kv, l, d = _iq4_fields(b, t)
        dl = np.repeat(d.astype(np.float32)[:, None] * l.astype(np.float32), 32, axis=1)
        out = dl * kv.astype(np.float32)
    elif t in (GGMLType.Q4_K, GGMLType.Q5_K):
        d = b[:, 0:2].copy().view(np.float16).astype(np.float32)
        dmin = b[:, 2:4].copy().view(np.float16).astype(np.float32)
        sc, m = _unpack_scale_min_k4(b[:, 4:16])
        if t == GGMLType.Q4_K:
            qs = b[:, 16:144]
            qh = None
        else:
            qh = b[:, 16:48]
            qs = b[:, 48:176]
        out = np.empty((nb, 256), np.float32)
        for j in range(4):
            grp = qs[:, 32 * j:32 * j + 32]
            lo = (grp & 0xF).astype(np.float32)
            hi = (grp >> 4).astype(np.float32)
            if qh is not None:
                lo += ((qh >> (2 * j)) & 1).astype(np.float32) * 16
                hi += ((qh >> (2 * j + 1)) & 1).astype(np.float32) * 16
            d1 = d[:, 0] * sc[:, 2 * j]
            m1 = dmin[:, 0] * m[:, 2 * j]
            d2 = d[:, 0] * sc[:, 2 * j + 1]
            m2 = dmin[:, 0] * m[:, 2 * j + 1]
            out[:, 64 * j:64 * j + 32] = d1[:, None] * lo - m1[:, None]
            out[:, 64 * j + 32:64 * j + 64] = d2[:, None] * hi - m2[:, None]
    elif t == GGMLType.Q6_K:
        ql = b[:, 0:128]
        qh = b[:, 128:192]
        scales = b[:, 192:208].view(np.int8).astype(np.float32)
        d = b[:, 208:210].copy().view(np.float16).astype(np.float32)[:, 0]
        out = np.empty((nb, 256), np.float32)
        for n in range(2):
            l_ = ql[:, 64 * n:64 * n + 64]
            h_ = qh[:, 32 * n:32 * n + 32]
            sc = scales[:, 8 * n:8 * n + 8]
            q1 = ((l_[:, 0:32] & 0xF) | (((h_ >> 0) & 3) << 4)).astype(np.float32) - 32
            q2 = ((l_[:, 32:64] & 0xF) | (((h_ >> 2) & 3) << 4)).astype(np.float32) - 32
            q3 = ((l_[:, 0:32] >> 4) | (((h_ >> 4) & 3) << 4)).astype(np.float32) - 32
            q4 = ((l_[:, 32:64] >> 4) | (((h_ >> 6) & 3) << 4)).astype(np.float32) - 32
            base = 128 * n
            for k, q in enumerate((q1, q2, q3, q4)):
                # 32 weights; scale index is = l/16 -> two scales per 32-run
                s = np.repeat(sc[:, [2 * k, 2 * k + 1]], 16, axis=1)
                out[:, base + 32 * k:base + 32 * k + 32] = d[:, None] * s * q
    else:
        raise NotImplementedError(f"dequantize {t.name}")
    out = out.reshape(-1)
    if n_elements is not None:
        assert out.size == n_elements
    return out

def _dequantize_f16(data, t, n_elements):
    b = _blocks(data, t)
    nb = b.shape[0]
    h = lambda v: np.asarray(v, np.float64).astype(np.float16).astype(np.float64)  # noqa: E731
    if t == GGMLType.Q8_0:
        d = b[:, 0:2].copy().view(np.float16).astype(np.float64)
        q = b[:, 2:34].view(np.int8).astype(np.float64)
        out = h(d * q)
    elif t in LEGACY_TYPES:
        # the tile16 copy stores (d, -8d) / (d, -16d) / (d, m) as an f16 pair per block
        d, m, q = _legacy_fields(b, t)
        a = d.astype(np.float64)
        off = h(-_legacy_offset(t) * a) if m is None else m.astype(np.float64)
        out = h(q.astype(np.float64) * a[:, None] + off[:, None])
    elif t in K23_TYPES:
        # the tile16 copy stores f16(d*sc) (f32 product) and, for Q2_K, f16(-dmin*m) per sub-block
        q, sc, m, d, dmin = _k23_fields(b, t)
        f32 = lambda v: np.asarray(v, np.float32)  # noqa: E731
        a = np.repeat(h(f32(d)[:, None] * f32(sc)), 16, axis=1)
        off = 0.0 if m is None else np.repeat(h(-f32(dmin)[:, None] * f32(m)), 16, axis=1)
        out = h(q.astype(np.float64) * a + off)
    elif t in IQ4_TYPES:
        # the tile16 copy stores f16(d*(ls-32)) per sub-block (IQ4_NL: d itself)
        kv, l, d = _iq4_fields(b, t)
        a = np.repeat(h(np.asarray(d, np.float32)[:, None] * np.asarray(l, np.float32)), 32, axis=1)
        out = h(kv.astype(np.float64) * a)
    elif t in (GGMLType.Q4_K, GGMLType.Q5_K):
        d = b[:, 0:2].copy().view(np.float16).astype(np.float64)[:, 0]
        dmin = b[:, 2:4].copy().view(np.float16).astype(np.float64)[:, 0]
        sc, m = _unpack_scale_min_k4(b[:, 4:16])
        qs = b[:, 16:144] if t == GGMLType.Q4_K else b[:, 48:176]
        qh = None if t == GGMLType.Q4_K else b[:, 16:48]
        out = np.empty((nb, 256), np.float64)
        for j in range(4):
            grp = qs[:, 32 * j:32 * j + 32]
            lo = (grp & 0xF).astype(np.float64)
            hi = (grp >> 4).astype(np.float64)
            if qh is not None:
                lo += ((qh >> (2 * j)) & 1).astype(np.float64) * 16
                hi += ((qh >> (2 * j + 1)) & 1).astype(np.float64) * 16
            for half, q in ((0, lo), (1, hi)):
                sb = 2 * j + half
                a = h(d * sc[:, sb])
                mn = h(-dmin * m[:, sb])
                out[:, 64 * j + 32 * half:64 * j + 32 * half + 32] = h(q * a[:, None] + mn[:, None])
    else:  # Q6_K
        ql = b[:, 0:128]
        qh = b[:, 128:192]
        scales = b[:, 192:208].view(np.int8).astype(np.float64)
        d = b[:, 208:210].copy().view(np.float16).astype(np.float64)[:, 0]
        out = np.empty((nb, 256), np.float64)
        for n in range(2):
            l_ = ql[:, 64 * n:64 * n + 64]
            h_ = qh[:, 32 * n:32 * n + 32]
            sc = scales[:, 8 * n:8 * n + 8]
            q1 = ((l_[:, 0:32] & 0xF) | (((h_ >> 0) & 3) << 4)).astype(np.float64) - 32
            q2 = ((l_[:, 32:64] & 0xF) | (((h_ >> 2) & 3) << 4)).astype(np.float64) - 32
            q3 = ((l_[:, 0:32] >> 4) | (((h_ >> 4) & 3) << 4)).astype(np.float64) - 32
            q4 = ((l_[:, 32:64] >> 4) | (((h_ >> 6) & 3) << 4)).astype(np.float64) - 32
            for k, q in enumerate((q1, q2, q3, q4)):
                a = np.repeat(h(d[:, None] * sc[:, [2 * k, 2 * k + 1]]), 16, axis=1)
                out[:, 128 * n + 32 * k:128 * n + 32 * k + 32] = h(q * a)
    out = out.reshape(-1).astype(np.float32)
    if n_elements is not None:
        assert out.size == n_elements
    return out

# --------------------------------------------------------------- quantise


def quantize(x: np.ndarray, ggml_type) -> np.ndarray:
    """Encode float32 (flat, length multiple of the block) -> raw bytes (uint8)."""
    t = GGMLType(ggml_type)
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    if t == GGMLType.F32:
        return x.view(np.uint8).copy()
    if t == GGMLType.F16:
        return x.astype(np.float16).view(np.uint8).copy()
    if t == GGMLType.BF16:
        u = x.view(np.uint32)
        r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
        return r.view(np.uint8).copy()
    if t == GGMLType.Q8_0:
        xb = x.reshape(-1, 32)
        amax = np.abs(xb).max(axis=1)
        d = amax / 127.0
        inv = np.where(d > 0, 1.0 / np.where(d > 0, d, 1), 0)
        q = np.clip(np.rint(xb * inv[:, None]), -127, 127).astype(np.int8)
        out = np.empty((xb.shape[0], 34), np.uint8)
        out[:, 0:2] = _f16(d).reshape(-1, 1).view(np.uint8)
        out[:, 2:] = q.view(np.uint8)
        return out.reshape(-1)
    if t in LEGACY_TYPES:
        nmax = 15 if t in (GGMLType.Q4_0, GGMLType.Q4_1) else 31
        xb = x.reshape(-1, 32)
        nb = xb.shape[0]
        if t in (GGMLType.Q4_0, GGMLType.Q5_0):
            # ggml: the value of largest magnitude maps to the most negative level
            off = _legacy_offset(t)
            vmax = np.take_along_axis(xb, np.argmax(np.abs(xb), axis=1)[:, None], axis=1)[:, 0]
            d16 = _f16(vmax / -off)
            m16 = None
            df = d16.astype(np.float32)
            inv = np.where(df != 0, 1.0 / np.where(df != 0, df, 1), 0)
            q = np.clip(np.rint(xb * inv[:, None]) + off, 0, nmax).astype(np.uint8)
        else:
            mn = xb.min(axis=1)
            d16 = _f16((xb.max(axis=1) - mn) / nmax)
            m16 = _f16(mn)
            df = d16.astype(np.float32)
            inv = np.where(df > 0, 1.0 / np.where(df > 0, df, 1), 0)
            q = np.clip(np.rint((xb - m16.astype(np.float32)[:, None]) * inv[:, None]), 0, nmax).astype(np.uint8)
        cols = [d16.reshape(-1, 1).view(np.uint8)]
        if m16 is not None:
            cols.append(m16.reshape(-1, 1).view(np.uint8))
        if nmax == 31:
            qh = (((q >> 4) & 1).astype(np.uint32) << np.arange(32, dtype=np.uint32)[None, :]).sum(
                axis=1, dtype=np.uint32)
            cols.append(qh.astype("<u4").reshape(-1, 1).view(np.uint8))
        cols.append((q[:, :16] & 0xF) | ((q[:, 16:] & 0xF) << 4))
        return np.concatenate(cols, axis=1).reshape(-1)
    if t in (GGMLType.Q4_K, GGMLType.Q5_K):
        nmax = 15 if t == GGMLType.Q4_K else 31
        xb = x.reshape(-1, 8, 32)
        mn = np.minimum(xb.min(axis=2), 0.0)          # [nb,8]  (min <= 0)
        mx = xb.max(axis=2)
        scale = (mx - mn) / nmax                      # per sub-block
        minv = -mn                                    # >= 0
        d = scale.max(axis=1) / 63.0                  # super-block scales
        dmin = minv.max(axis=1) / 63.0
        d16 = _f16(d).astype(np.float32)
        dm16 = _f16(dmin).astype(np.float32)
        sc = np.clip(np.rint(np.where(d16[:, None] > 0, scale / np.where(d16 > 0, d16, 1)[:, None], 0)), 0, 63)
        m = np.clip(np.rint(np.where(dm16[:, None] > 0, minv / np.where(dm16 > 0, dm16, 1)[:, None], 0)), 0, 63)
        eff_s = d16[:, None] * sc
        eff_m = dm16[:, None] * m
        q = np.where(eff_s[:, :, None] > 0,
                     np.rint((xb + eff_m[:, :, None]) / np.where(eff_s > 0, eff_s, 1)[:, :, None]), 0)
        q = np.clip(q, 0, nmax).astype(np.uint8)       # [nb,8,32]
        nb = xb.shape[0]
        packed = _pack_scale_min_k4(sc.astype(np.uint8), m.astype(np.uint8))
        qs = np.empty((nb, 128), np.uint8)
        for j in range(4):
            qs[:, 32 * j:32 * j + 32] = (q[:, 2 * j] & 0xF) | ((q[:, 2 * j + 1] & 0xF) << 4)
        head = np.empty((nb, 4), np.uint8)
        head[:, 0:2] = _f16(d).reshape(-1, 1).view(np.uint8)
        head[:, 2:4] = _f16(dmin).reshape(-1, 1).view(np.uint8)
        if t == GGMLType.Q4_K:
            return np.concatenate([head, packed, qs], axis=1).reshape(-1)
        qh = np.zeros((nb, 32), np.uint8)
        for j in range(8):
            qh |= ((q[:, j] >> 4) & 1).astype(np.uint8) << j
        return np.concatenate([head, packed, qh, qs], axis=1).reshape(-1)
    if t == GGMLType.Q2_K:
        # per 16-weight sub-block min/max; 4-bit scale and min against the block's d / dmin
        xb = x.reshape(-1, 16, 16)
        mn = np.minimum(xb.min(axis=2), 0.0)
        scale = (xb.max(axis=2) - mn) / 3.0
        minv = -mn
        d16 = _f16(scale.max(axis=1) / 15.0)
        dm16 = _f16(minv.max(axis=1) / 15.0)
        df, dmf = d16.astype(np.float32), dm16.astype(np.float32)
        sc = np.clip(np.rint(np.where(df[:, None] > 0, scale / np.where(df > 0, df, 1)[:, None], 0)), 0, 15)
        m = np.clip(np.rint(np.where(dmf[:, None] > 0, minv / np.where(dmf > 0, dmf, 1)[:, None], 0)), 0, 15)
        eff_s = df[:, None] * sc
        eff_m = dmf[:, None] * m
        q = np.where(eff_s[:, :, None] > 0,
                     np.rint((xb + eff_m[:, :, None]) / np.where(eff_s > 0, eff_s, 1)[:, :, None]), 0)
        q = np.clip(q, 0, 3).astype(np.uint8).reshape(-1, 256)
        scales = (sc.astype(np.uint8) | (m.astype(np.uint8) << 4))
        return np.concatenate([scales, _pack_2bit(q), d16.reshape(-1, 1).view(np.uint8),
                               dm16.reshape(-1, 1).view(np.uint8)], axis=1).reshape(-1)
    if t == GGMLType.Q3_K:
        # per 16-weight sub-block absmax (signed, as Q6_K: the extreme value maps to -4); 6-bit scales
        xb = x.reshape(-1, 16, 16)
        vmax = np.take_along_axis(xb, np.argmax(np.abs(xb), axis=2)[:, :, None], axis=2)[:, :, 0]
        scale = -vmax / 4.0
        smax = np.take_along_axis(scale, np.argmax(np.abs(scale), axis=1)[:, None], axis=1)[:, 0]
        iscale = np.where(smax != 0, -32.0 / np.where(smax != 0, smax, 1), 0)
        d = np.where(iscale != 0, 1.0 / np.where(iscale != 0, iscale, 1), 0)
        d16 = _f16(d)
        sc = np.clip(np.rint(iscale[:, None] * scale), -32, 31).astype(np.int16)
        eff = d16.astype(np.float32)[:, None] * sc.astype(np.float32)
        q = np.where(eff[:, :, None] != 0, np.rint(xb / np.where(eff != 0, eff, 1)[:, :, None]), 0)
        q = (np.clip(q, -4, 3) + 4).astype(np.uint8).reshape(-1, 256)
        hmask = np.zeros((q.shape[0], 32), np.uint8)
        for n in range(2):
            for j in range(4):
                hmask |= ((q[:, 128 * n + 32 * j:128 * n + 32 * j + 32] >> 2) & 1).astype(np.uint8) << (4 * n + j)
        return np.concatenate([hmask, _pack_2bit(q), _pack_q3k_scales((sc + 32).astype(np.uint8)),
                               d16.reshape(-1, 1).view(np.uint8)], axis=1).reshape(-1)
    if t == GGMLType.IQ4_NL:
        # the weight of largest magnitude maps to the codebook's -127 (d takes its sign, flipped)
        xb = x.reshape(-1, 32).astype(np.float64)
        vmax = np.take_along_axis(xb, np.argmax(np.abs(xb), axis=1)[:, None], axis=1)[:, 0]
        d16 = _f16(vmax / -127.0 + 0.0)  # (+ 0.0: an all-zero block gets +0, not -0)
        df = d16.astype(np.float64)
        q = np.where(df[:, None] != 0, _iq4_nearest(xb / np.where(df != 0, df, 1)[:, None]), 8).astype(np.uint8)
        return np.concatenate([d16.reshape(-1, 1).view(np.uint8), q[:, :16] | (q[:, 16:] << 4)], axis=1).reshape(-1)
    if t == GGMLType.IQ4_XS:
        # per 32-weight sub-block the IQ4_NL scale; the largest of them is the block's -32 and the
        # others are truncated towards zero against it (6 bits), so that every sub-block's extreme
        # weight still lands on the codebook's -127 and a second pass finds the same d, scales
        # and indices (quantize o dequantize is a fixed point)
        xb = x.reshape(-1, 8, 32).astype(np.float64)
        vmax = np.take_along_axis(xb, np.argmax(np.abs(xb), axis=2)[:, :, None], axis=2)[:, :, 0]
        scale = vmax / -127.0
        smax = np.take_along_axis(scale, np.argmax(np.abs(scale), axis=1)[:, None], axis=1)[:, 0]
        d = smax / -32.0 + 0.0
        d16 = _f16(d)
        l = np.clip(np.trunc(np.where(d[:, None] != 0, scale / np.where(d != 0, d, 1)[:, None], 0)), -32, 31)
        eff = d16.astype(np.float64)[:, None] * l
        q = np.where(eff[:, :, None] != 0, _iq4_nearest(xb / np.where(eff != 0, eff, 1)[:, :, None]), 8).astype(np.uint8)
        ls = (l + 32).astype(np.uint8)
        sl = (ls[:, 0::2] & 15) | ((ls[:, 1::2] & 15) << 4)
        sh = np.zeros(ls.shape[0], np.uint16)
        for ib in range(8):
            sh |= (ls[:, ib] >> 4).astype(np.uint16) << (2 * ib)
        qs = (q[:, :, :16] | (q[:, :, 16:] << 4)).reshape(-1, 128)
        return np.concatenate([d16.reshape(-1, 1).view(np.uint8), sh.astype("<u2").reshape(-1, 1).view(np.uint8),
                               sl, qs], axis=1).reshape(-1)
    if t == GGMLType.Q6_K:
        xb = x.reshape(-1, 16, 16)
        amax_idx = np.argmax(np.abs(xb), axis=2)
        vmax = np.take_along_axis(xb, amax_idx[:, :, None], axis=2)[:, :, 0]
        scale = -vmax / 32.0                           # ggml uses the signed max
        smax_idx = np.argmax(np.abs(scale), axis=1)
        smax = np.take_along_axis(scale, smax_idx[:, None], axis=1)[:, 0]
        iscale = np.where(smax != 0, -128.0 / np.where(smax != 0, smax, 1), 0)
        d = np.where(iscale != 0, 1.0 / np.where(iscale != 0, iscale, 1), 0)
        d16 = _f16(d).astype(np.float32)
        sc = np.clip(np.rint(iscale[:, None] * scale), -128, 127).astype(np.int8)
        eff = d16[:, None] * sc.astype(np.float32)
        q = np.where(eff[:, :, None] != 0, np.rint(xb / np.where(eff != 0, eff, 1)[:, :, None]), 0)
        q = (np.clip(q, -32, 31) + 32).astype(np.uint8).reshape(-1, 256)
        nb = q.shape[0]
        ql = np.empty((nb, 128), np.uint8)
        qh = np.empty((nb, 64), np.uint8)
        for n in range(2):
            qq = q[:, 128 * n:128 * n + 128]
            for l in range(32):
                q1, q2, q3, q4 = qq[:, l], qq[:, l + 32], qq[:, l + 64], qq[:, l + 96]
                ql[:, 64 * n + l] = (q1 & 0xF) | ((q3 & 0xF) << 4)
                ql[:, 64 * n + l + 32] = (q2 & 0xF) | ((q4 & 0xF) << 4)
                qh[:, 32 * n + l] = (q1 >> 4) | ((q2 >> 4) << 2) | ((q3 >> 4) << 4) | ((q4 >> 4) << 6)
        out = np.concatenate([ql, qh, sc.view(np.uint8), _f16(d).reshape(-1, 1).view(np.uint8)], axis=1)
        return out.reshape(-1)
    raise NotImplementedError(f"quantize {t.name}")

# ------------------------------------------------------- synthetic blocks


def random_blocks(ggml_type, n_elements: int, rng: np.random.Generator, std: float = 0.02) -> np.ndarray:
    """Valid random blocks of ``ggml_type`` whose decoded weights have roughly
    zero mean and standard deviation ``std`` - generated directly in the block
    domain (random quants + bounded f16 scales), no float->quant pass, so a
    multi-GB synthetic GGUF streams out at memory speed."""
    t = GGMLType(ggml_type)
    bs, bb = GGML_BLOCK[t]
    nb = n_elements // bs
    if t == GGMLType.F32:
        return (rng.standard_normal(n_elements, dtype=np.float32) * std).view(np.uint8)
    if t in (GGMLType.F16, GGMLType.BF16):
        return quantize(rng.standard_normal(n_elements, dtype=np.float32) * std, t)
    raw = np.frombuffer(rng.bytes(nb * bb), dtype=np.uint8).reshape(nb, bb).copy()
    if t == GGMLType.Q8_0:
        # q uniform in [-128,127] -> rms ~73.9
        d = np.full(nb, std / 73.9, np.float32) * rng.uniform(0.5, 1.5, nb).astype(np.float32)
        raw[:, 0:2] = _f16(d).reshape(-1, 1).view(np.uint8)
    elif t in (GGMLType.Q4_K, GGMLType.Q5_K):
        nmax = 15 if t == GGMLType.Q4_K else 31
        # sc, m uniform in [0,63]; q uniform in [0,nmax]. dmin = d*nmax/2 centres w.
        var_sq = (63 * 127 / 6) * (nmax * (2 * nmax + 1) / 6) - (31.5 * nmax / 2) ** 2
        var = var_sq + (nmax / 2) ** 2 * (64 ** 2 - 1) / 12
        d = np.full(nb, std / np.sqrt(var), np.float32) * rng.uniform(0.5, 1.5, nb).astype(np.float32)
        raw[:, 0:2] = _f16(d).reshape(-1, 1).view(np.uint8)
        raw[:, 2:4] = _f16(d * nmax / 2).reshape(-1, 1).view(np.uint8)
    elif t in LEGACY_TYPES:
        # q uniform in [0, nmax]: variance (nmax + 1)^2 / 12 (the offset or m centres it)
        nmax = 15 if t in (GGMLType.Q4_0, GGMLType.Q4_1) else 31
        d = np.full(nb, std / np.sqrt(((nmax + 1) ** 2 - 1) / 12.0), np.float32) * \
            rng.uniform(0.5, 1.5, nb).astype(np.float32)
        raw[:, 0:2] = _f16(d).reshape(-1, 1).view(np.uint8)
        if t in (GGMLType.Q4_1, GGMLType.Q5_1):
            raw[:, 2:4] = _f16(-d * nmax / 2).reshape(-1, 1).view(np.uint8)
    elif t == GGMLType.Q2_K:
        # sc, m uniform in [0,15]; q uniform in [0,3]; dmin = 1.5 d centres w:
        # var = E[sc^2] E[q^2] - (E[sc] E[q])^2 + 1.5^2 var(m)
        var = (15 * 31 / 6) * 3.5 - (7.5 * 1.5) ** 2 + 2.25 * (16 ** 2 - 1) / 12
        d = np.full(nb, std / np.sqrt(var), np.float32) * rng.uniform(0.5, 1.5, nb).astype(np.float32)
        raw[:, 80:82] = _f16(d).reshape(-1, 1).view(np.uint8)
        raw[:, 82:84] = _f16(d * 1.5).reshape(-1, 1).view(np.uint8)
    elif t == GGMLType.Q3_K:
        # sc - 32 uniform in [-32,31] (mean square 341.5); q uniform in [-4,3] (mean square 5.5)
        d = np.full(nb, std / np.sqrt(341.5 * 5.5), np.float32) * rng.uniform(0.5, 1.5, nb).astype(np.float32)
        raw[:, 108:110] = _f16(d).reshape(-1, 1).view(np.uint8)
    elif t == GGMLType.Q6_K:
        # scales int8 uniform [-128,127] (rms ~73.9); q-32 uniform [-32,31] (rms ~18.5)
        d = np.full(nb, std / (73.9 * 18.5), np.float32) * rng.uniform(0.5, 1.5, nb).astype(np.float32)
        raw[:, 208:210] = _f16(d).reshape(-1, 1).view(np.uint8)
    elif t == GGMLType.IQ4_NL:
        # codebook index uniform: mean square 4548; the codebook's mean is -5.875, so d takes a
        # random sign (a negative d is what the quantiser writes for a positive extreme weight)
        d = np.full(nb, std / np.sqrt(4548.0), np.float32) * rng.uniform(0.5, 1.5, nb).astype(np.float32)
        d *= rng.choice(np.array([-1.0, 1.0], np.float32), nb)
        raw[:, 0:2] = _f16(d).reshape(-1, 1).view(np.uint8)
    elif t == GGMLType.IQ4_XS:
        # ls - 32 uniform in [-32,31] (mean square 341.5, mean -0.5: the weights are centred)
        d = np.full(nb, std / np.sqrt(341.5 * 4548.0), np.float32) * rng.uniform(0.5, 1.5, nb).astype(np.float32)
        raw[:, 0:2] = _f16(d).reshape(-1, 1).view(np.uint8)
    else:
        raise NotImplementedError(t.name)
    return raw.reshape(-1)
