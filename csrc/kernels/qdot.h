// Device-side block decoding for the planar weight layout (see ../common.h).
//
// Unit of work = one "chunk" = 32 weights of one row = 16 B of 4/6-bit data.
// A row of K weights has K/32 chunks; lane l of a wave takes chunks l, l+64, ...
// The activation vector is pre-quantised to int8 with one f32 scale per 32
// values (q8 activations, as llama.cpp's MMVQ path), so the inner product is
// int8 x int8 on v_dot4c_i32_i8 (4 MACs per VALU op) and the per-sub-block
// scales are applied once per 16-32 weights.
//
// Chunk c -> which x elements it multiplies (per superblock sb = c>>3):
//   Q4_K/Q5_K : j=c&7, g=j>>1, h=j&1 : lo 16 @ sb*256+64g+16h (sub-block 2g),
//                                      hi 16 @ +32               (sub-block 2g+1)
//   Q6_K      : j=c&7, n=j>>2, o=16(j&3): lo 16 @ sb*256+128n+o, hi 16 @ +64
//   Q8_0/F16/F32: 32 contiguous @ 32c
//   Q4_0/Q4_1/Q5_0/Q5_1: chunk c = block c, 32 contiguous @ 32c like Q8_0: the low nibbles
//                        are weights 32c .. 32c+15, the high nibbles 32c+16 .. 32c+31
//   Q2_K/Q3_K : the x map of Q4_K: j=c&7, g=j>>1, h=j&1 : lo 16 @ sb*256+64g+16h (sub-block 4g+h),
//               hi 16 @ +32 (sub-block 4g+h+2). A 16-byte quant load of these formats carries 64
//               weights - the 16-runs at +0, +32, +64, +96 of half n = g>>1, in bit pairs 0..3 of
//               bytes 32n+16h .. +15 - so chunks g = 2n and 2n+1 of one h read the SAME 16 bytes
//               and take bit pairs (0, 1) and (2, 3): one shift by 4(g&1) / 4(g&1)+2 and a
//               0x03030303 mask per dword. The two lanes' loads fall in one 64-byte line of one
//               load instruction, so HBM streams every byte once; Q3_K's hmask bytes 16h .. +15
//               (bit 4n+2(g&1) / +1) are shared by four chunks the same way.
//   IQ4_NL/IQ4_XS: chunk c = 32 contiguous weights @ 32c like Q8_0 (IQ4_NL: block c; IQ4_XS:
//               sub-block c & 7 of superblock c >> 3), Q4_0's nibble order; a nibble is an index
//               into the 16-entry signed codebook (iq4_lookup), so there is no min / offset term
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include "../common.h"

namespace lfk {

// two f32 -> packed bf16 pair in ONE v_cvt_pk_bf16_f32 (round to nearest even); the scalar
// __float2bfloat16 form costs a conversion per value plus the shift/or to pack
typedef float f32x2_pk_t __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2_pk_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pk_bf16_pair(float a, float b) {
  const f32x2_pk_t v = {a, b};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_pk_t));
}

__device__ __forceinline__ float h2f(unsigned short h) {
  return __half2float(__ushort_as_half(h));
}

typedef int i32x4_t __attribute__((ext_vector_type(4)));

// the XCD (XCC) this wave runs on, for timeline stamps (per-XCD clocks; placement tools only)
__device__ __forceinline__ unsigned xcc_id() { return __builtin_amdgcn_s_getreg(20 | (0 << 6) | (15 << 11)); }

// 16-B non-temporal load (weights are streamed once per token: do not pollute L2/MALL)
__device__ __forceinline__ int4 ld_nt16(const void* p) {
  const i32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const i32x4_t*>(p));
  return make_int4(v.x, v.y, v.z, v.w);
}

__device__ __forceinline__ int dot4(int a, int b, int c) { return __builtin_amdgcn_sdot4(a, b, c, false); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// ---- cross-lane reductions without the LDS crossbar (DPP within 16-lane rows,
// v_readlane across rows): a few cycles per step instead of a ds_bpermute trip.
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float max8(float v) {   // max over each aligned group of 8 lanes
  v = fmaxf(v, dpp_f<0xB1>(v));                      // quad_perm [1,0,3,2]
  v = fmaxf(v, dpp_f<0x4E>(v));                      // quad_perm [2,3,0,1]
  return fmaxf(v, dpp_f<0x141>(v));                  // row_half_mirror
}
__device__ __forceinline__ float row_sum16(float v) {  // sum over each 16-lane row
  v += dpp_f<0xB1>(v);
  v += dpp_f<0x4E>(v);
  v += dpp_f<0x141>(v);
  return v + dpp_f<0x140>(v);                        // row_mirror
}
__device__ __forceinline__ float readlane_f(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
__device__ __forceinline__ float wave_max_fast(float v) {  // wave-uniform result
  v = fmaxf(v, dpp_f<0xB1>(v));
  v = fmaxf(v, dpp_f<0x4E>(v));
  v = fmaxf(v, dpp_f<0x141>(v));
  v = fmaxf(v, dpp_f<0x140>(v));
  return fmaxf(fmaxf(readlane_f(v, 0), readlane_f(v, 16)), fmaxf(readlane_f(v, 32), readlane_f(v, 48)));
}
__device__ __forceinline__ float wave_sum_fast(float v) {  // wave-uniform result
  v = row_sum16(v);
  return (readlane_f(v, 0) + readlane_f(v, 16)) + (readlane_f(v, 32) + readlane_f(v, 48));
}

// x operand of one chunk, read once from LDS and reused across the NR rows.
struct XChunk {
  int lo[4];
  int hi[4];
  float dlo, dhi;  // x scales
  float slo, shi;  // x scale * sum(q_x) over the 16 lo / hi values (for the min / -32 terms)
};

template <int T>
__device__ __forceinline__ void load_x(XChunk& X, const int8_t* xq, const float* xd, int c) {
  const int sb = c >> 3, j = c & 7;
  int off_lo, off_hi, blo, bhi;
  if constexpr (T == T_Q4_K || T == T_Q5_K || T == T_Q2_K || T == T_Q3_K) {
    const int g = j >> 1, h = j & 1;
    off_lo = sb * 256 + 64 * g + 16 * h;
    off_hi = off_lo + 32;
    blo = sb * 8 + 2 * g;
    bhi = blo + 1;
  } else if constexpr (T == T_Q6_K) {
    const int n = j >> 2, o = 16 * (j & 3);
    off_lo = sb * 256 + 128 * n + o;
    off_hi = off_lo + 64;
    blo = off_lo >> 5;
    bhi = blo + 2;
  } else {  // Q8_0 / legacy 32-blocks / F16 / F32: 32 contiguous values = one x block
    off_lo = 32 * c;
    off_hi = off_lo + 16;
    blo = bhi = c;
  }
  const int4 a = *reinterpret_cast<const int4*>(xq + off_lo);
  const int4 b = *reinterpret_cast<const int4*>(xq + off_hi);
  X.lo[0] = a.x; X.lo[1] = a.y; X.lo[2] = a.z; X.lo[3] = a.w;
  X.hi[0] = b.x; X.hi[1] = b.y; X.hi[2] = b.z; X.hi[3] = b.w;
  X.dlo = xd[blo];
  X.dhi = xd[bhi];
  const int ones = 0x01010101;
  int s0 = dot4(X.lo[0], ones, dot4(X.lo[1], ones, dot4(X.lo[2], ones, dot4(X.lo[3], ones, 0))));
  int s1 = dot4(X.hi[0], ones, dot4(X.hi[1], ones, dot4(X.hi[2], ones, dot4(X.hi[3], ones, 0))));
  X.slo = X.dlo * (float)s0;
  X.shi = X.dhi * (float)s1;
}

// ---- legacy 32-weight blocks (Q4_0 / Q4_1 / Q5_0 / Q5_1): w = d * q + m with m = -8d / -16d
// for the symmetric types. One raw form for all four: the 16 quant bytes, the 5-bit types' high
// bits and the scale field (d, or d | m << 16).
template <int T> inline constexpr bool is_legacy_v = (T == T_Q4_0 || T == T_Q4_1 || T == T_Q5_0 || T == T_Q5_1);
template <int T> inline constexpr bool legacy_has_m = (T == T_Q4_1 || T == T_Q5_1);
template <int T> inline constexpr bool legacy_has_h = (T == T_Q5_0 || T == T_Q5_1);
struct LegacyRaw {
  int4 q;
  unsigned h, s;
};

// block c of a row: plane row pointers p0 (qs), p1 and p2 as planes_of orders them
template <int T, bool NT>
__device__ __forceinline__ void legacy_load(LegacyRaw& w, const uint8_t* p0, const uint8_t* p1, const uint8_t* p2,
                                            int c) {
  if constexpr (NT) w.q = ld_nt16(p0 + 16 * c);
  else w.q = *reinterpret_cast<const int4*>(p0 + 16 * c);
  const uint8_t* sp = legacy_has_h<T> ? p2 : p1;
  if constexpr (legacy_has_h<T>) w.h = *reinterpret_cast<const unsigned*>(p1 + 4 * c);
  else w.h = 0u;
  if constexpr (legacy_has_m<T>) w.s = *reinterpret_cast<const unsigned*>(sp + 4 * c);
  else w.s = *reinterpret_cast<const unsigned short*>(sp + 2 * c);
}

template <int T>
__device__ __forceinline__ void legacy_scale(const LegacyRaw& w, float& d, float& m) {
  d = h2f(w.s & 0xFFFF);
  if constexpr (legacy_has_m<T>) m = h2f(w.s >> 16);
  else m = (T == T_Q4_0 ? -8.f : -16.f) * d;
}

// quant dword i (i = 0..3) as bytes: lo = weights 4i .. 4i+3, hi = weights 16+4i .. 16+4i+3.
// 5-bit types: the four qh bits of a dword are spread to bit 0 of its four bytes by one 24-bit
// multiply (bit k lands on 8k; the partial products meet no other bit, so nothing carries).
template <int T>
__device__ __forceinline__ void legacy_quants(const LegacyRaw& w, int i, int& lo, int& hi) {
  const unsigned q = (unsigned)(i == 0 ? w.q.x : i == 1 ? w.q.y : i == 2 ? w.q.z : w.q.w);
  unsigned l = q & 0x0F0F0F0Fu, h = (q >> 4) & 0x0F0F0F0Fu;
  if constexpr (legacy_has_h<T>) {
    const unsigned bl = __umul24((w.h >> (4 * i)) & 0xFu, 0x00204081u) & 0x01010101u;
    const unsigned bh = __umul24((w.h >> (16 + 4 * i)) & 0xFu, 0x00204081u) & 0x01010101u;
    l |= bl << 4;
    h |= bh << 4;
  }
  lo = (int)l;
  hi = (int)h;
}

template <int T>
__device__ __forceinline__ float legacy_dot(const LegacyRaw& w, const XChunk& X) {
  int acc = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int lo, hi;
    legacy_quants<T>(w, i, lo, hi);
    acc = dot4(lo, X.lo[i], acc);
    acc = dot4(hi, X.hi[i], acc);
  }
  float d, m;
  legacy_scale<T>(w, d, m);
  // sum((d q + m) x) = d * dot + m * sum(x): the offset / min goes through the x sums
  return d * (X.dlo * (float)acc) + m * (X.slo + X.shi);
}

template <int T>
__device__ __forceinline__ void legacy_decode(const LegacyRaw& w, float* out) {
  float d, m;
  legacy_scale<T>(w, d, m);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int lo, hi;
    legacy_quants<T>(w, i, lo, hi);
#pragma unroll
    for (int b8 = 0; b8 < 4; ++b8) {
      out[4 * i + b8] = d * (float)((lo >> (8 * b8)) & 0xFF) + m;
      out[16 + 4 * i + b8] = d * (float)((hi >> (8 * b8)) & 0xFF) + m;
    }
  }
}

// ---- 2- and 3-bit K-quants (Q2_K / Q3_K): 16 sub-blocks of 16 weights, so each 16-run of a chunk
// has its own scale. Q2_K: w = d (sc & 15) q - dmin (sc >> 4), q in 0..3. Q3_K: w = d (sc6 - 32)
// (q - 4), q = 2 low bits | hmask bit << 2. The min and the -4 go through the x sums.
template <int T> inline constexpr bool is_k23_v = (T == T_Q2_K || T == T_Q3_K);

// Q3_K's 6-bit scale of sub-block s, minus 32, from the 12 packed bytes as three dwords
__device__ __forceinline__ int q3k_sc(unsigned s0, unsigned s1, unsigned s2, int s) {
  const unsigned v = (s & 4) ? s1 : s0;
  const unsigned low = (v >> (8 * (s & 3) + 4 * (s >> 3))) & 0xFu;
  const unsigned top = (s2 >> (8 * (s & 3) + 2 * (s >> 2))) & 3u;
  return (int)(low | (top << 4)) - 32;
}

// one chunk's raw fields (GEMV)
struct K23Raw {
  int4 q;               // qs bytes 32n + 16h .. +15 of the block
  int4 h;               // Q3_K: hmask bytes 16h .. +15
  unsigned s0, s1, s2;  // Q2_K: the scale bytes of the low / high run (s2 unused); Q3_K: the 12 packed bytes
  unsigned d;           // Q2_K: d | dmin << 16; Q3_K: d
};

template <int T, bool NT>
__device__ __forceinline__ void k23_load(K23Raw& w, const uint8_t* p0, const uint8_t* p1, const uint8_t* p2,
                                         const uint8_t* p3, int c) {
  const int sb = c >> 3, j = c & 7, g = j >> 1, hh = j & 1;
  const uint8_t* qp = p0 + 64 * sb + 32 * (g >> 1) + 16 * hh;
  if constexpr (NT) w.q = ld_nt16(qp);
  else w.q = *reinterpret_cast<const int4*>(qp);
  if constexpr (T == T_Q2_K) {
    const uint8_t* sp = p1 + 16 * sb + 4 * g + hh;
    w.s0 = sp[0];
    w.s1 = sp[2];
    w.d = *reinterpret_cast<const unsigned*>(p2 + 4 * sb);
  } else {
    w.h = *reinterpret_cast<const int4*>(p1 + 32 * sb + 16 * hh);
    const unsigned* sp = reinterpret_cast<const unsigned*>(p2 + 12 * sb);
    w.s0 = sp[0];
    w.s1 = sp[1];
    w.s2 = sp[2];
    w.d = *reinterpret_cast<const unsigned short*>(p3 + 2 * sb);
  }
}

template <int T>
__device__ __forceinline__ float k23_dot(const K23Raw& w, const XChunk& X, int c) {
  const int j = c & 7, g = j >> 1, hh = j & 1, sh = 4 * (g & 1);
  const int qv[4] = {w.q.x, w.q.y, w.q.z, w.q.w};
  int dl = 0, dh = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int lo = (qv[i] >> sh) & 0x03030303;
    int hi = (qv[i] >> (sh + 2)) & 0x03030303;
    if constexpr (T == T_Q3_K) {
      const int hv = (i == 0 ? w.h.x : i == 1 ? w.h.y : i == 2 ? w.h.z : w.h.w);
      const int b = 2 * g;  // bit 4n + 2e of the hmask byte = bit 2g
      lo |= ((hv >> b) & 0x01010101) << 2;
      hi |= ((hv >> (b + 1)) & 0x01010101) << 2;
    }
    dl = dot4(lo, X.lo[i], dl);
    dh = dot4(hi, X.hi[i], dh);
  }
  if constexpr (T == T_Q2_K) {
    const float d = h2f(w.d & 0xFFFF), dmin = h2f(w.d >> 16);
    return d * ((float)(w.s0 & 0xF) * X.dlo * (float)dl + (float)(w.s1 & 0xF) * X.dhi * (float)dh) -
           dmin * ((float)(w.s0 >> 4) * X.slo + (float)(w.s1 >> 4) * X.shi);
  } else {
    const int s = 4 * g + hh;
    const float sc_lo = (float)q3k_sc(w.s0, w.s1, w.s2, s), sc_hi = (float)q3k_sc(w.s0, w.s1, w.s2, s + 2);
    // sum((q - 4) x) = dot - 4 sum(x)
    return h2f(w.d & 0xFFFF) * (sc_lo * (X.dlo * (float)dl - 4.f * X.slo) + sc_hi * (X.dhi * (float)dh - 4.f * X.shi));
  }
}

// 32 contiguous weights (run r = q & 7 of a block: half n = r >> 2, bit pair r & 3, sub-blocks 2r, 2r + 1)
struct K23Dq {
  int4 a, b;            // qs bytes 32n .. +31
  int4 ha, hb;          // Q3_K: hmask[32]
  unsigned s0, s1, s2;  // Q2_K: s0 = the two scale bytes of sub-blocks 2r, 2r + 1; Q3_K: the 12 packed bytes
  unsigned d;
};

template <int T>
__device__ __forceinline__ void k23_dq_load(K23Dq& w, const uint8_t* __restrict__ base, const Planes& P, size_t row,
                                            int q) {
  const int sb = q >> 3, r = q & 7;
  const int4* qs = reinterpret_cast<const int4*>(base + P.p0 + row * P.s0 + 64 * sb + 32 * (r >> 2));
  w.a = qs[0];
  w.b = qs[1];
  if constexpr (T == T_Q2_K) {
    w.s0 = *reinterpret_cast<const unsigned short*>(base + P.p1 + row * P.s1 + 16 * sb + 2 * r);
    w.d = *reinterpret_cast<const unsigned*>(base + P.p2 + row * P.s2 + 4 * sb);
  } else {
    const int4* hm = reinterpret_cast<const int4*>(base + P.p1 + row * P.s1 + 32 * sb);
    w.ha = hm[0];
    w.hb = hm[1];
    const unsigned* sp = reinterpret_cast<const unsigned*>(base + P.p2 + row * P.s2 + 12 * sb);
    w.s0 = sp[0];
    w.s1 = sp[1];
    w.s2 = sp[2];
    w.d = *reinterpret_cast<const unsigned short*>(base + P.p3 + row * P.s3 + 2 * sb);
  }
}

template <int T>
__device__ __forceinline__ void k23_dq_decode(const K23Dq& w, int q, float* out) {
  const int r = q & 7, sh = 2 * (r & 3);
  const int qv[8] = {w.a.x, w.a.y, w.a.z, w.a.w, w.b.x, w.b.y, w.b.z, w.b.w};
  float a0, a1, m0, m1;
  if constexpr (T == T_Q2_K) {
    const float d = h2f(w.d & 0xFFFF), dmin = h2f(w.d >> 16);
    a0 = d * (float)(w.s0 & 0xF); m0 = dmin * (float)((w.s0 >> 4) & 0xF);
    a1 = d * (float)((w.s0 >> 8) & 0xF); m1 = dmin * (float)(w.s0 >> 12);
  } else {
    const float d = h2f(w.d & 0xFFFF);
    a0 = d * (float)q3k_sc(w.s0, w.s1, w.s2, 2 * r);
    a1 = d * (float)q3k_sc(w.s0, w.s1, w.s2, 2 * r + 1);
    m0 = m1 = 0.f;
  }
  const int hv[8] = {w.ha.x, w.ha.y, w.ha.z, w.ha.w, w.hb.x, w.hb.y, w.hb.z, w.hb.w};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    int v = (qv[i] >> sh) & 0x03030303;
    if constexpr (T == T_Q3_K) v |= ((hv[i] >> r) & 0x01010101) << 2;  // bit 4n + j of the byte = bit r
#pragma unroll
    for (int b8 = 0; b8 < 4; ++b8) {
      const int qq = (v >> (8 * b8)) & 0xFF;
      if constexpr (T == T_Q2_K) out[4 * i + b8] = (i < 4 ? a0 : a1) * (float)qq - (i < 4 ? m0 : m1);
      else out[4 * i + b8] = (i < 4 ? a0 : a1) * (float)(qq - 4);
    }
  }
}

// ---- non-linear 4-bit (IQ4_NL / IQ4_XS): w = d * kIQ4Values[nibble] (IQ4_XS: d * (ls - 32) with the
// sub-block's 6-bit ls). The codebook is signed, so the dot is scale * dx * acc with no offset term.
template <int T> inline constexpr bool is_iq4_v = (T == T_IQ4_NL || T == T_IQ4_XS);

// dword i of the codebook (entries 4i .. 4i + 3, one per byte), every byte xor `flip`: 0 gives the
// signed bytes v_dot4 takes, 0x80 gives value + 128 as an unsigned byte (bmm.hip's f16 magic)
constexpr unsigned iq4_table_dword(int i, unsigned flip) {
  unsigned v = 0;
  for (int b = 0; b < 4; ++b) v |= ((unsigned)(uint8_t)kIQ4Values[4 * i + b] ^ flip) << (8 * b);
  return v;
}

// The codebook bytes of a quant dword's four low nibbles (lo) and four high nibbles (hi).
// v_perm_b32 picks each result byte from 8 source bytes, the table has 16: one permute looks
// the index's low three bits up in entries 0..7, one in entries 8..15, and a third takes byte k
// from the second result where bit 3 of index k is set (selector k + 4) and from the first
// otherwise (selector k). Per 4 weights: and, 2 perm, shift, and-or, perm (+ a shift for hi);
// the table's four dwords and the masks are constants the compiler keeps in registers.
template <unsigned FLIP>
__device__ __forceinline__ void iq4_lookup(unsigned q, unsigned& lo, unsigned& hi) {
  constexpr unsigned T0 = iq4_table_dword(0, FLIP), T1 = iq4_table_dword(1, FLIP);
  constexpr unsigned T2 = iq4_table_dword(2, FLIP), T3 = iq4_table_dword(3, FLIP);
  const unsigned sl = q & 0x07070707u, sh = (q >> 4) & 0x07070707u;
  const unsigned pl = ((q >> 1) & 0x04040404u) | 0x03020100u, ph = ((q >> 5) & 0x04040404u) | 0x03020100u;
  lo = __builtin_amdgcn_perm(__builtin_amdgcn_perm(T3, T2, sl), __builtin_amdgcn_perm(T1, T0, sl), pl);
  hi = __builtin_amdgcn_perm(__builtin_amdgcn_perm(T3, T2, sh), __builtin_amdgcn_perm(T1, T0, sh), ph);
}

// one chunk's raw fields: the 16 quant bytes and the scale field(s) -
// IQ4_NL: s0 = d; IQ4_XS: s0 = d | scales_h << 16, s1 = scales_l[4] (the superblock's 8 bytes)
struct IQ4Raw {
  int4 q;
  unsigned s0, s1;
};

// chunk c of a row: plane row pointers p0 (qs) and p1 (d / sc)
template <int T, bool NT>
__device__ __forceinline__ void iq4_load(IQ4Raw& w, const uint8_t* p0, const uint8_t* p1, int c) {
  if constexpr (NT) w.q = ld_nt16(p0 + 16 * c);
  else w.q = *reinterpret_cast<const int4*>(p0 + 16 * c);
  if constexpr (T == T_IQ4_NL) {
    w.s0 = *reinterpret_cast<const unsigned short*>(p1 + 2 * c);
    w.s1 = 0u;
  } else {
    const uint2 m = *reinterpret_cast<const uint2*>(p1 + 8 * (c >> 3));
    w.s0 = m.x;
    w.s1 = m.y;
  }
}

// the chunk's scale: d, or d * (ls - 32) with ls = nibble ib of scales_l | bit pair ib of scales_h << 4
template <int T>
__device__ __forceinline__ float iq4_scale(const IQ4Raw& w, int c) {
  const float d = h2f(w.s0 & 0xFFFF);
  if constexpr (T == T_IQ4_NL) {
    return d;
  } else {
    const int ib = c & 7;
    const unsigned ls = ((w.s1 >> (4 * ib)) & 0xFu) | ((((w.s0 >> 16) >> (2 * ib)) & 3u) << 4);
    return d * (float)((int)ls - 32);
  }
}

template <int T>
__device__ __forceinline__ float iq4_dot(const IQ4Raw& w, const XChunk& X, int c) {
  const unsigned qv[4] = {(unsigned)w.q.x, (unsigned)w.q.y, (unsigned)w.q.z, (unsigned)w.q.w};
  int acc = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    unsigned lo, hi;
    iq4_lookup<0u>(qv[i], lo, hi);
    acc = dot4((int)lo, X.lo[i], acc);
    acc = dot4((int)hi, X.hi[i], acc);
  }
  return iq4_scale<T>(w, c) * (X.dlo * (float)acc);
}

template <int T>
__device__ __forceinline__ void iq4_decode(const IQ4Raw& w, int c, float* out) {
  const float sc = iq4_scale<T>(w, c);
  const unsigned qv[4] = {(unsigned)w.q.x, (unsigned)w.q.y, (unsigned)w.q.z, (unsigned)w.q.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    unsigned lo, hi;
    iq4_lookup<0u>(qv[i], lo, hi);
#pragma unroll
    for (int b8 = 0; b8 < 4; ++b8) {
      out[4 * i + b8] = sc * (float)(signed char)((lo >> (8 * b8)) & 0xFF);
      out[16 + 4 * i + b8] = sc * (float)(signed char)((hi >> (8 * b8)) & 0xFF);
    }
  }
}

// 6-bit (sc, m) pair for sub-blocks 2g and 2g+1 from the 12 packed scale bytes (ggml get_scale_min_k4).
__device__ __forceinline__ void scale_min_pair(int g, unsigned y, unsigned z, unsigned w, float& sc_lo, float& m_lo,
                                               float& sc_hi, float& m_hi) {
  // g < 2: direct 6-bit fields; g >= 2: 4 low bits in w, 2 high bits in the top of y / z.
  const int k = (g & 1) * 16;  // byte offset*8 of sub-block 2g within its dword (g=0,2 -> 0; 1,3 -> 16)
  unsigned a_sc, a_m, b_sc, b_m;
  if (g < 2) {
    a_sc = (y >> k) & 63;
    b_sc = (y >> (k + 8)) & 63;
    a_m = (z >> k) & 63;
    b_m = (z >> (k + 8)) & 63;
  } else {
    a_sc = ((w >> k) & 0xF) | (((y >> (k + 6)) & 3) << 4);
    b_sc = ((w >> (k + 8)) & 0xF) | (((y >> (k + 14)) & 3) << 4);
    a_m = ((w >> (k + 4)) & 0xF) | (((z >> (k + 6)) & 3) << 4);
    b_m = ((w >> (k + 12)) & 0xF) | (((z >> (k + 14)) & 3) << 4);
  }
  sc_lo = (float)a_sc; m_lo = (float)a_m; sc_hi = (float)b_sc; m_hi = (float)b_m;
}

template <int T>
__device__ __forceinline__ float chunk_dot(const uint8_t* __restrict__ base, const Planes& P, size_t row, int c,
                                           const XChunk& X) {
  const int sb = c >> 3, j = c & 7;
  if constexpr (T == T_Q4_K || T == T_Q5_K) {
    const int g = j >> 1;
    const uint8_t* qs_p = base + P.p0 + row * P.s0 + 16 * c;
    int4 q = ld_nt16(qs_p);
    int4 meta, qh;
    if constexpr (T == T_Q4_K) {
      meta = *reinterpret_cast<const int4*>(base + P.p1 + row * P.s1 + sb * 16);
    } else {
      qh = *reinterpret_cast<const int4*>(base + P.p1 + row * P.s1 + sb * 32 + 16 * (j & 1));
      meta = *reinterpret_cast<const int4*>(base + P.p2 + row * P.s2 + sb * 16);
    }
    const unsigned dd = (unsigned)meta.x;
    const float d = h2f(dd & 0xFFFF), dmin = h2f(dd >> 16);
    float sc_lo, m_lo, sc_hi, m_hi;
    scale_min_pair(g, (unsigned)meta.y, (unsigned)meta.z, (unsigned)meta.w, sc_lo, m_lo, sc_hi, m_hi);
    const int qv[4] = {q.x, q.y, q.z, q.w};
    int dl = 0, dh = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int lo = qv[i] & 0x0F0F0F0F;
      int hi = (qv[i] >> 4) & 0x0F0F0F0F;
      if constexpr (T == T_Q5_K) {
        const int hv = (i == 0 ? qh.x : i == 1 ? qh.y : i == 2 ? qh.z : qh.w);
        lo |= ((hv >> (2 * g)) & 0x01010101) << 4;
        hi |= ((hv >> (2 * g + 1)) & 0x01010101) << 4;
      }
      dl = dot4(lo, X.lo[i], dl);
      dh = dot4(hi, X.hi[i], dh);
    }
    return d * (sc_lo * X.dlo * (float)dl + sc_hi * X.dhi * (float)dh) - dmin * (m_lo * X.slo + m_hi * X.shi);
  } else if constexpr (T == T_Q6_K) {
    const int n = j >> 2, o = 16 * (j & 3);
    int4 ql = ld_nt16(base + P.p0 + row * P.s0 + 16 * c);
    int4 qh = *reinterpret_cast<const int4*>(base + P.p1 + row * P.s1 + sb * 64 + 32 * n + (o & 31));
    int4 scv = *reinterpret_cast<const int4*>(base + P.p2 + row * P.s2 + sb * 16);
    const float d = h2f(*reinterpret_cast<const unsigned short*>(base + P.p3 + row * P.s3 + sb * 2));
    const int si = 8 * n + (o >> 4);  // lo scale index; hi = si + 4
    const int scw[4] = {scv.x, scv.y, scv.z, scv.w};
    const int sc_lo = (int)(signed char)((scw[si >> 2] >> (8 * (si & 3))) & 0xFF);
    const int sc_hi = (int)(signed char)((scw[(si + 4) >> 2] >> (8 * (si & 3))) & 0xFF);
    const int s = (o >= 32) ? 2 : 0;
    const int lv[4] = {ql.x, ql.y, ql.z, ql.w};
    const int hv[4] = {qh.x, qh.y, qh.z, qh.w};
    int dl = 0, dh = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int lo = (lv[i] & 0x0F0F0F0F) | (((hv[i] >> s) & 0x03030303) << 4);
      const int hi = ((lv[i] >> 4) & 0x0F0F0F0F) | (((hv[i] >> (s + 4)) & 0x03030303) << 4);
      dl = dot4(lo, X.lo[i], dl);
      dh = dot4(hi, X.hi[i], dh);
    }
    // sum((q-32) x) = dot - 32*sum(x)
    return d * ((float)sc_lo * (X.dlo * (float)dl - 32.f * X.slo) + (float)sc_hi * (X.dhi * (float)dh - 32.f * X.shi));
  } else if constexpr (T == T_Q8_0) {
    const int4* qp = reinterpret_cast<const int4*>(base + P.p0 + row * P.s0 + 32 * c);
    int4 a = ld_nt16(qp);
    int4 b = ld_nt16(qp + 1);
    const float d = h2f(*reinterpret_cast<const unsigned short*>(base + P.p1 + row * P.s1 + 2 * c));
    int acc = dot4(a.x, X.lo[0], 0);
    acc = dot4(a.y, X.lo[1], acc);
    acc = dot4(a.z, X.lo[2], acc);
    acc = dot4(a.w, X.lo[3], acc);
    acc = dot4(b.x, X.hi[0], acc);
    acc = dot4(b.y, X.hi[1], acc);
    acc = dot4(b.z, X.hi[2], acc);
    acc = dot4(b.w, X.hi[3], acc);
    return d * X.dlo * (float)acc;
  } else if constexpr (is_legacy_v<T>) {
    LegacyRaw w;
    legacy_load<T, true>(w, base + P.p0 + row * P.s0, base + P.p1 + row * P.s1, base + P.p2 + row * P.s2, c);
    return legacy_dot<T>(w, X);
  } else if constexpr (is_k23_v<T>) {
    K23Raw w;
    k23_load<T, true>(w, base + P.p0 + row * P.s0, base + P.p1 + row * P.s1, base + P.p2 + row * P.s2,
                      base + P.p3 + row * P.s3, c);
    return k23_dot<T>(w, X, c);
  } else if constexpr (is_iq4_v<T>) {
    IQ4Raw w;
    iq4_load<T, true>(w, base + P.p0 + row * P.s0, base + P.p1 + row * P.s1, c);
    return iq4_dot<T>(w, X, c);
  } else {  // F32 / F16 weights: dequantised x
    static_assert(T == T_F32 || T == T_F16, "chunk_dot: unsupported type");
    float s = 0.f;
    const int xv[8] = {X.lo[0], X.lo[1], X.lo[2], X.lo[3], X.hi[0], X.hi[1], X.hi[2], X.hi[3]};
    if constexpr (T == T_F32) {
      const float4* wp = reinterpret_cast<const float4*>(base + row * P.s0 + 128 * c);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        float4 w = wp[i];
        const int v = xv[i];
        s += w.x * (float)(signed char)(v & 0xFF) + w.y * (float)(signed char)((v >> 8) & 0xFF) +
             w.z * (float)(signed char)((v >> 16) & 0xFF) + w.w * (float)(signed char)((v >> 24) & 0xFF);
      }
    } else {
      const uint2* wp = reinterpret_cast<const uint2*>(base + row * P.s0 + 64 * c);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        uint2 w = wp[i];
        const int v = xv[i];
        s += h2f(w.x & 0xFFFF) * (float)(signed char)(v & 0xFF) + h2f(w.x >> 16) * (float)(signed char)((v >> 8) & 0xFF) +
             h2f(w.y & 0xFFFF) * (float)(signed char)((v >> 16) & 0xFF) + h2f(w.y >> 16) * (float)(signed char)((v >> 24) & 0xFF);
      }
    }
    return s * X.dlo;
  }
}

// ---------------------------------------------------------------------------
// Split load / compute form of chunk_dot: the GEMV issues the loads of ALL its
// rows x passes first (WRaw), then does the integer math, so every lane keeps
// NR x 2 independent 16-B loads in flight instead of one at a time.
template <int T> struct WRaw;
template <> struct WRaw<T_Q4_K> { int4 q, m; };
template <> struct WRaw<T_Q5_K> { int4 q, h, m; };
template <> struct WRaw<T_Q6_K> { int4 l, h; int slo, shi; unsigned d; };
template <> struct WRaw<T_Q8_0> { int4 a, b; unsigned d; };
template <> struct WRaw<T_Q4_0> : LegacyRaw {};
template <> struct WRaw<T_Q4_1> : LegacyRaw {};
template <> struct WRaw<T_Q5_0> : LegacyRaw {};
template <> struct WRaw<T_Q5_1> : LegacyRaw {};
template <> struct WRaw<T_Q2_K> : K23Raw {};
template <> struct WRaw<T_Q3_K> : K23Raw {};
template <> struct WRaw<T_IQ4_NL> : IQ4Raw {};
template <> struct WRaw<T_IQ4_XS> : IQ4Raw {};
template <> struct WRaw<T_F16> { uint4 w[4]; };
template <> struct WRaw<T_F32> { float4 w[8]; };

// per-row plane pointers (wave-uniform -> SGPRs)
struct RowPtr {
  const uint8_t* p0;
  const uint8_t* p1;
  const uint8_t* p2;
  const uint8_t* p3;
};

__device__ __forceinline__ RowPtr row_ptr(const uint8_t* base, const Planes& P, unsigned row) {
  RowPtr r;
  r.p0 = base + P.p0 + (size_t)row * P.s0;
  r.p1 = base + P.p1 + (size_t)row * P.s1;
  r.p2 = base + P.p2 + (size_t)row * P.s2;
  r.p3 = base + P.p3 + (size_t)row * P.s3;
  return r;
}

template <int T>
__device__ __forceinline__ void wload(WRaw<T>& w, const RowPtr& R, int c) {
  const int sb = c >> 3, j = c & 7;
  if constexpr (T == T_Q4_K) {
    w.q = ld_nt16(R.p0 + 16 * c);
    w.m = *reinterpret_cast<const int4*>(R.p1 + 16 * sb);
  } else if constexpr (T == T_Q5_K) {
    w.q = ld_nt16(R.p0 + 16 * c);
    w.h = *reinterpret_cast<const int4*>(R.p1 + 32 * sb + 16 * (j & 1));
    w.m = *reinterpret_cast<const int4*>(R.p2 + 16 * sb);
  } else if constexpr (T == T_Q6_K) {
    const int n = j >> 2, o = 16 * (j & 3);
    w.l = ld_nt16(R.p0 + 16 * c);
    w.h = *reinterpret_cast<const int4*>(R.p1 + 64 * sb + 32 * n + (o & 31));
    const int si = 8 * n + (o >> 4);
    w.slo = *reinterpret_cast<const signed char*>(R.p2 + 16 * sb + si);
    w.shi = *reinterpret_cast<const signed char*>(R.p2 + 16 * sb + si + 4);
    w.d = *reinterpret_cast<const unsigned short*>(R.p3 + 2 * sb);
  } else if constexpr (T == T_Q8_0) {
    w.a = ld_nt16(R.p0 + 32 * c);
    w.b = ld_nt16(R.p0 + 32 * c + 16);
    w.d = *reinterpret_cast<const unsigned short*>(R.p1 + 2 * c);
  } else if constexpr (is_legacy_v<T>) {
    legacy_load<T, true>(w, R.p0, R.p1, R.p2, c);
  } else if constexpr (is_k23_v<T>) {
    k23_load<T, true>(w, R.p0, R.p1, R.p2, R.p3, c);
  } else if constexpr (is_iq4_v<T>) {
    iq4_load<T, true>(w, R.p0, R.p1, c);
  } else if constexpr (T == T_F16) {
#pragma unroll
    for (int i = 0; i < 4; ++i) w.w[i] = reinterpret_cast<const uint4*>(R.p0 + 64 * c)[i];
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) w.w[i] = reinterpret_cast<const float4*>(R.p0 + 128 * c)[i];
  }
}

template <int T>
__device__ __forceinline__ float wdot(const WRaw<T>& w, const XChunk& X, int c) {
  const int j = c & 7;
  if constexpr (T == T_Q4_K || T == T_Q5_K) {
    const int g = j >> 1;
    const unsigned dd = (unsigned)w.m.x;
    const float d = h2f(dd & 0xFFFF), dmin = h2f(dd >> 16);
    float sc_lo, m_lo, sc_hi, m_hi;
    scale_min_pair(g, (unsigned)w.m.y, (unsigned)w.m.z, (unsigned)w.m.w, sc_lo, m_lo, sc_hi, m_hi);
    const int qv[4] = {w.q.x, w.q.y, w.q.z, w.q.w};
    int dl = 0, dh = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int lo = qv[i] & 0x0F0F0F0F;
      int hi = (qv[i] >> 4) & 0x0F0F0F0F;
      if constexpr (T == T_Q5_K) {
        const int hv = (i == 0 ? w.h.x : i == 1 ? w.h.y : i == 2 ? w.h.z : w.h.w);
        lo |= ((hv >> (2 * g)) & 0x01010101) << 4;
        hi |= ((hv >> (2 * g + 1)) & 0x01010101) << 4;
      }
      dl = dot4(lo, X.lo[i], dl);
      dh = dot4(hi, X.hi[i], dh);
    }
    return d * (sc_lo * X.dlo * (float)dl + sc_hi * X.dhi * (float)dh) - dmin * (m_lo * X.slo + m_hi * X.shi);
  } else if constexpr (T == T_Q6_K) {
    const int o = 16 * (j & 3);
    const int sc_lo = w.slo, sc_hi = w.shi;
    const int s = (o >= 32) ? 2 : 0;
    const int lv[4] = {w.l.x, w.l.y, w.l.z, w.l.w};
    const int hv[4] = {w.h.x, w.h.y, w.h.z, w.h.w};
    int dl = 0, dh = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int lo = (lv[i] & 0x0F0F0F0F) | (((hv[i] >> s) & 0x03030303) << 4);
      const int hi = ((lv[i] >> 4) & 0x0F0F0F0F) | (((hv[i] >> (s + 4)) & 0x03030303) << 4);
      dl = dot4(lo, X.lo[i], dl);
      dh = dot4(hi, X.hi[i], dh);
    }
    const float d = h2f(w.d & 0xFFFF);
    return d * ((float)sc_lo * (X.dlo * (float)dl - 32.f * X.slo) + (float)sc_hi * (X.dhi * (float)dh - 32.f * X.shi));
  } else if constexpr (T == T_Q8_0) {
    int acc = dot4(w.a.x, X.lo[0], 0);
    acc = dot4(w.a.y, X.lo[1], acc);
    acc = dot4(w.a.z, X.lo[2], acc);
    acc = dot4(w.a.w, X.lo[3], acc);
    acc = dot4(w.b.x, X.hi[0], acc);
    acc = dot4(w.b.y, X.hi[1], acc);
    acc = dot4(w.b.z, X.hi[2], acc);
    acc = dot4(w.b.w, X.hi[3], acc);
    return h2f(w.d & 0xFFFF) * X.dlo * (float)acc;
  } else if constexpr (is_legacy_v<T>) {
    return legacy_dot<T>(w, X);
  } else if constexpr (is_k23_v<T>) {
    return k23_dot<T>(w, X, c);
  } else if constexpr (is_iq4_v<T>) {
    return iq4_dot<T>(w, X, c);
  } else {
    static_assert(T == T_F32 || T == T_F16, "wdot: unsupported type");
    const int xv[8] = {X.lo[0], X.lo[1], X.lo[2], X.lo[3], X.hi[0], X.hi[1], X.hi[2], X.hi[3]};
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int v = xv[i];
      const float x0 = (float)(signed char)(v & 0xFF), x1 = (float)(signed char)((v >> 8) & 0xFF);
      const float x2 = (float)(signed char)((v >> 16) & 0xFF), x3 = (float)(signed char)((v >> 24) & 0xFF);
      if constexpr (T == T_F32) {
        const float4 ww = w.w[i];
        s += ww.x * x0 + ww.y * x1 + ww.z * x2 + ww.w * x3;
      } else {
        const uint2 ww = (i & 1) ? make_uint2(w.w[i >> 1].z, w.w[i >> 1].w) : make_uint2(w.w[i >> 1].x, w.w[i >> 1].y);
        s += h2f(ww.x & 0xFFFF) * x0 + h2f(ww.x >> 16) * x1 + h2f(ww.y & 0xFFFF) * x2 + h2f(ww.y >> 16) * x3;
      }
    }
    return s * X.dlo;
  }
}

// Dequantise 32 CONTIGUOUS weights [32*q, 32*q+32) of `row` into out[32] (used by
// the embedding gather and the prefill GEMM's LDS staging).
template <int T>
__device__ __forceinline__ void dequant32(const uint8_t* __restrict__ base, const Planes& P, size_t row, int q,
                                          float* out) {
  if constexpr (T == T_Q4_K || T == T_Q5_K) {
    const int sb = q >> 3, s = q & 7, g = s >> 1, hi = s & 1;  // sub-block s of superblock sb
    const uint8_t* qs_p = base + P.p0 + row * P.s0 + sb * 128 + 32 * g;
    int4 meta;
    int4 qh0, qh1;
    if constexpr (T == T_Q4_K) {
      meta = *reinterpret_cast<const int4*>(base + P.p1 + row * P.s1 + sb * 16);
    } else {
      const int4* qhp = reinterpret_cast<const int4*>(base + P.p1 + row * P.s1 + sb * 32);
      qh0 = qhp[0];
      qh1 = qhp[1];
      meta = *reinterpret_cast<const int4*>(base + P.p2 + row * P.s2 + sb * 16);
    }
    const float d = h2f((unsigned)meta.x & 0xFFFF), dmin = h2f((unsigned)meta.x >> 16);
    float sc_lo, m_lo, sc_hi, m_hi;
    scale_min_pair(g, (unsigned)meta.y, (unsigned)meta.z, (unsigned)meta.w, sc_lo, m_lo, sc_hi, m_hi);
    const float scl = d * (hi ? sc_hi : sc_lo), mn = dmin * (hi ? m_hi : m_lo);
    const int4 a = reinterpret_cast<const int4*>(qs_p)[0];
    const int4 b = reinterpret_cast<const int4*>(qs_p)[1];
    const int qv[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    const int hv[8] = {qh0.x, qh0.y, qh0.z, qh0.w, qh1.x, qh1.y, qh1.z, qh1.w};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      int v = hi ? ((qv[i] >> 4) & 0x0F0F0F0F) : (qv[i] & 0x0F0F0F0F);
      if constexpr (T == T_Q5_K) v |= ((hv[i] >> s) & 0x01010101) << 4;
#pragma unroll
      for (int b8 = 0; b8 < 4; ++b8) out[4 * i + b8] = scl * (float)((v >> (8 * b8)) & 0xFF) - mn;
    }
  } else if constexpr (T == T_Q6_K) {
    const int sb = q >> 3, r = q & 7;        // 32-run r of the superblock
    const int n = r >> 2, qq = (r >> 1) & 1, half = r & 1;
    const uint8_t* qlp = base + P.p0 + row * P.s0 + sb * 128 + 64 * n + 32 * half;
    const uint8_t* qhp = base + P.p1 + row * P.s1 + sb * 64 + 32 * n;
    const int4 scv = *reinterpret_cast<const int4*>(base + P.p2 + row * P.s2 + sb * 16);
    const float d = h2f(*reinterpret_cast<const unsigned short*>(base + P.p3 + row * P.s3 + sb * 2));
    const int scw[4] = {scv.x, scv.y, scv.z, scv.w};
    const int si = 8 * n + 2 * (2 * qq + half);
    const float s0 = d * (float)(signed char)((scw[si >> 2] >> (8 * (si & 3))) & 0xFF);
    const float s1 = d * (float)(signed char)((scw[(si + 1) >> 2] >> (8 * ((si + 1) & 3))) & 0xFF);
    const int4 la = reinterpret_cast<const int4*>(qlp)[0], lb = reinterpret_cast<const int4*>(qlp)[1];
    const int4 ha = reinterpret_cast<const int4*>(qhp)[0], hb = reinterpret_cast<const int4*>(qhp)[1];
    const int lv[8] = {la.x, la.y, la.z, la.w, lb.x, lb.y, lb.z, lb.w};
    const int hv[8] = {ha.x, ha.y, ha.z, ha.w, hb.x, hb.y, hb.z, hb.w};
    const int hs = 2 * (2 * qq + half);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int v = ((lv[i] >> (4 * qq)) & 0x0F0F0F0F) | (((hv[i] >> hs) & 0x03030303) << 4);
#pragma unroll
      for (int b8 = 0; b8 < 4; ++b8) out[4 * i + b8] = (i < 4 ? s0 : s1) * (float)(((v >> (8 * b8)) & 0xFF) - 32);
    }
  } else if constexpr (T == T_Q8_0) {
    const int4* qp = reinterpret_cast<const int4*>(base + P.p0 + row * P.s0 + 32 * q);
    const int4 a = qp[0], b = qp[1];
    const float d = h2f(*reinterpret_cast<const unsigned short*>(base + P.p1 + row * P.s1 + 2 * q));
    const int qv[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int b8 = 0; b8 < 4; ++b8) out[4 * i + b8] = d * (float)(signed char)((qv[i] >> (8 * b8)) & 0xFF);
  } else if constexpr (is_legacy_v<T>) {
    LegacyRaw w;
    legacy_load<T, false>(w, base + P.p0 + row * P.s0, base + P.p1 + row * P.s1, base + P.p2 + row * P.s2, q);
    legacy_decode<T>(w, out);
  } else if constexpr (is_k23_v<T>) {
    K23Dq w;
    k23_dq_load<T>(w, base, P, row, q);
    k23_dq_decode<T>(w, q, out);
  } else if constexpr (is_iq4_v<T>) {
    IQ4Raw w;
    iq4_load<T, false>(w, base + P.p0 + row * P.s0, base + P.p1 + row * P.s1, q);
    iq4_decode<T>(w, q, out);
  } else if constexpr (T == T_F32) {
    const float4* wp = reinterpret_cast<const float4*>(base + row * P.s0 + 128 * q);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float4 w = wp[i];
      out[4 * i] = w.x; out[4 * i + 1] = w.y; out[4 * i + 2] = w.z; out[4 * i + 3] = w.w;
    }
  } else {  // F16
    const uint2* wp = reinterpret_cast<const uint2*>(base + row * P.s0 + 64 * q);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      uint2 w = wp[i];
      out[4 * i] = h2f(w.x & 0xFFFF); out[4 * i + 1] = h2f(w.x >> 16);
      out[4 * i + 2] = h2f(w.y & 0xFFFF); out[4 * i + 3] = h2f(w.y >> 16);
    }
  }
}

// ---------------------------------------------------------------------------
// Split form of dequant32 for software-pipelined GEMM staging: dq_load issues
// the raw loads of one 32-weight run (registers), dq_decode turns them into 32
// floats later, so the loads of K-step k+1 fly while step k's MFMAs run.
template <int T> struct DqRaw;
template <> struct DqRaw<T_Q4_K> { int4 a, b, m; };
template <> struct DqRaw<T_Q5_K> { int4 a, b, m, h0, h1; };
template <> struct DqRaw<T_Q6_K> { int4 la, lb, ha, hb, sc; unsigned d; };
template <> struct DqRaw<T_Q8_0> { int4 a, b; unsigned d; };
template <> struct DqRaw<T_Q4_0> : LegacyRaw {};
template <> struct DqRaw<T_Q4_1> : LegacyRaw {};
template <> struct DqRaw<T_Q5_0> : LegacyRaw {};
template <> struct DqRaw<T_Q5_1> : LegacyRaw {};
template <> struct DqRaw<T_Q2_K> : K23Dq {};
template <> struct DqRaw<T_Q3_K> : K23Dq {};
template <> struct DqRaw<T_IQ4_NL> : IQ4Raw {};
template <> struct DqRaw<T_IQ4_XS> : IQ4Raw {};
template <> struct DqRaw<T_F16> { uint4 w[4]; };
template <> struct DqRaw<T_F32> { float4 w[8]; };

template <int T>
__device__ __forceinline__ void dq_load(DqRaw<T>& r, const uint8_t* __restrict__ base, const Planes& P, size_t row,
                                        int q) {
  if constexpr (T == T_Q4_K || T == T_Q5_K) {
    const int sb = q >> 3, g = (q & 7) >> 1;
    const int4* qs = reinterpret_cast<const int4*>(base + P.p0 + row * P.s0 + sb * 128 + 32 * g);
    r.a = qs[0];
    r.b = qs[1];
    if constexpr (T == T_Q4_K) {
      r.m = *reinterpret_cast<const int4*>(base + P.p1 + row * P.s1 + sb * 16);
    } else {
      const int4* qh = reinterpret_cast<const int4*>(base + P.p1 + row * P.s1 + sb * 32);
      r.h0 = qh[0];
      r.h1 = qh[1];
      r.m = *reinterpret_cast<const int4*>(base + P.p2 + row * P.s2 + sb * 16);
    }
  } else if constexpr (T == T_Q6_K) {
    const int sb = q >> 3, rr = q & 7, n = rr >> 2, half = rr & 1;
    const int4* l = reinterpret_cast<const int4*>(base + P.p0 + row * P.s0 + sb * 128 + 64 * n + 32 * half);
    const int4* h = reinterpret_cast<const int4*>(base + P.p1 + row * P.s1 + sb * 64 + 32 * n);
    r.la = l[0]; r.lb = l[1];
    r.ha = h[0]; r.hb = h[1];
    r.sc = *reinterpret_cast<const int4*>(base + P.p2 + row * P.s2 + sb * 16);
    r.d = *reinterpret_cast<const unsigned short*>(base + P.p3 + row * P.s3 + sb * 2);
  } else if constexpr (T == T_Q8_0) {
    const int4* qp = reinterpret_cast<const int4*>(base + P.p0 + row * P.s0 + 32 * q);
    r.a = qp[0];
    r.b = qp[1];
    r.d = *reinterpret_cast<const unsigned short*>(base + P.p1 + row * P.s1 + 2 * q);
  } else if constexpr (is_legacy_v<T>) {
    legacy_load<T, false>(r, base + P.p0 + row * P.s0, base + P.p1 + row * P.s1, base + P.p2 + row * P.s2, q);
  } else if constexpr (is_k23_v<T>) {
    k23_dq_load<T>(r, base, P, row, q);
  } else if constexpr (is_iq4_v<T>) {
    iq4_load<T, false>(r, base + P.p0 + row * P.s0, base + P.p1 + row * P.s1, q);
  } else if constexpr (T == T_F16) {
#pragma unroll
    for (int i = 0; i < 4; ++i) r.w[i] = reinterpret_cast<const uint4*>(base + row * P.s0 + 64 * q)[i];
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) r.w[i] = reinterpret_cast<const float4*>(base + row * P.s0 + 128 * q)[i];
  }
}

template <int T>
__device__ __forceinline__ void dq_decode(const DqRaw<T>& r, int q, float* out) {
  if constexpr (T == T_Q4_K || T == T_Q5_K) {
    const int s = q & 7, hi = s & 1;
    const float d = h2f((unsigned)r.m.x & 0xFFFF), dmin = h2f((unsigned)r.m.x >> 16);
    // this lane's one 6-bit (scale, min) pair, branch-free (s differs per lane; a branch here
    // would also split the GEMM's MFMA/decode scheduling region)
    const unsigned y = r.m.y, z = r.m.z, w = r.m.w;
    const int sh = 8 * (s & 3);
    const unsigned sc_a = (y >> sh) & 63, m_a = (z >> sh) & 63;
    const unsigned sc_b = ((w >> sh) & 0xF) | (((y >> (sh + 6)) & 3) << 4);
    const unsigned m_b = ((w >> (sh + 4)) & 0xF) | (((z >> (sh + 6)) & 3) << 4);
    const float scl = d * (float)(s >= 4 ? sc_b : sc_a), mn = dmin * (float)(s >= 4 ? m_b : m_a);
    const int qv[8] = {r.a.x, r.a.y, r.a.z, r.a.w, r.b.x, r.b.y, r.b.z, r.b.w};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      int v = hi ? ((qv[i] >> 4) & 0x0F0F0F0F) : (qv[i] & 0x0F0F0F0F);
      if constexpr (T == T_Q5_K) {
        const int hv = i < 4 ? (i == 0 ? r.h0.x : i == 1 ? r.h0.y : i == 2 ? r.h0.z : r.h0.w)
                             : (i == 4 ? r.h1.x : i == 5 ? r.h1.y : i == 6 ? r.h1.z : r.h1.w);
        v |= ((hv >> s) & 0x01010101) << 4;
      }
#pragma unroll
      for (int b8 = 0; b8 < 4; ++b8) out[4 * i + b8] = scl * (float)((v >> (8 * b8)) & 0xFF) - mn;
    }
  } else if constexpr (T == T_Q6_K) {
    const int rr = q & 7, n = rr >> 2, qq = (rr >> 1) & 1, half = rr & 1;
    const float d = h2f(r.d & 0xFFFF);
    const int scw[4] = {r.sc.x, r.sc.y, r.sc.z, r.sc.w};
    const int si = 8 * n + 2 * (2 * qq + half);
    const float s0 = d * (float)(signed char)((scw[si >> 2] >> (8 * (si & 3))) & 0xFF);
    const float s1 = d * (float)(signed char)((scw[(si + 1) >> 2] >> (8 * ((si + 1) & 3))) & 0xFF);
    const int lv[8] = {r.la.x, r.la.y, r.la.z, r.la.w, r.lb.x, r.lb.y, r.lb.z, r.lb.w};
    const int hv[8] = {r.ha.x, r.ha.y, r.ha.z, r.ha.w, r.hb.x, r.hb.y, r.hb.z, r.hb.w};
    const int hs = 2 * (2 * qq + half);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int v = ((lv[i] >> (4 * qq)) & 0x0F0F0F0F) | (((hv[i] >> hs) & 0x03030303) << 4);
#pragma unroll
      for (int b8 = 0; b8 < 4; ++b8) out[4 * i + b8] = (i < 4 ? s0 : s1) * (float)(((v >> (8 * b8)) & 0xFF) - 32);
    }
  } else if constexpr (T == T_Q8_0) {
    const float d = h2f(r.d & 0xFFFF);
    const int qv[8] = {r.a.x, r.a.y, r.a.z, r.a.w, r.b.x, r.b.y, r.b.z, r.b.w};
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int b8 = 0; b8 < 4; ++b8) out[4 * i + b8] = d * (float)(signed char)((qv[i] >> (8 * b8)) & 0xFF);
  } else if constexpr (is_legacy_v<T>) {
    legacy_decode<T>(r, out);
  } else if constexpr (is_k23_v<T>) {
    k23_dq_decode<T>(r, q, out);
  } else if constexpr (is_iq4_v<T>) {
    iq4_decode<T>(r, q, out);
  } else if constexpr (T == T_F16) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned w[4] = {r.w[i].x, r.w[i].y, r.w[i].z, r.w[i].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        out[8 * i + 2 * j] = h2f(w[j] & 0xFFFF);
        out[8 * i + 2 * j + 1] = h2f(w[j] >> 16);
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      out[4 * i] = r.w[i].x; out[4 * i + 1] = r.w[i].y; out[4 * i + 2] = r.w[i].z; out[4 * i + 3] = r.w[i].w;
    }
  }
}

}  // namespace lfk
