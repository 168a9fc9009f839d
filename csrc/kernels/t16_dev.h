// Device-side pieces of the tile16 kernels shared by their translation units (bmm.hip: the batched
// decode projections and the prefill GEMM; score.hip: the scoring head): the raw-weight records of
// each step format, their dequantisation into v_mfma_f32_16x16x32_f16 A fragments, the x offsets
// of a chunk's runs, the raw loads from a tile16 step block and the LDS-only barrier. The layout
// itself is documented with t16_repack in bmm.hip.
#pragma once
#include "gemv_dev.h"

namespace lfk {

typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
typedef _Float16 h8_t __attribute__((ext_vector_type(8)));
typedef float f4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ h2_t as_h2(unsigned v) { return __builtin_bit_cast(h2_t, v); }
__device__ __forceinline__ unsigned as_u(h2_t v) { return __builtin_bit_cast(unsigned, v); }

// bytes 0 and 2 (or 1 and 3) of x under the f16 exponent of 1024: one v_perm_b32 builds the
// pair (1024 + b0, 1024 + b2) - the and / shift / or it replaces were 2-3 VALU ops per pair
// (the compiler did not form v_and_or_b32: CDNA VOP3 takes no literal constant)
__device__ __forceinline__ unsigned bytes02(unsigned x) { return __builtin_amdgcn_perm(0x64646464u, x, 0x04020400u); }
__device__ __forceinline__ unsigned bytes13(unsigned x) { return __builtin_amdgcn_perm(0x64646464u, x, 0x04030401u); }

// a (1024 + v0, 1024 + v1) f16 pair -> (v * a + m): exact subtraction of `bias`, one fma
__device__ __forceinline__ unsigned deq_pair(unsigned magic_pair, h2_t bias, h2_t a, h2_t m) {
  const h2_t v = as_h2(magic_pair) - bias;
  return as_u(v * a + m);
}

struct HFrag {
  unsigned w[16];  // MFMA i takes w[4i .. 4i+3]
};

// bmm's raw weights of one chunk: the WRaw layouts, except Q4_K, whose tile16 copy carries
// the sub-block scales pre-decoded - per row and sub-block one f16 pair (d * sc, -dmin * m) -
// instead of the packed 12-byte scales: the 6-bit unpacking was ~40 VALU ops per chunk, about
// a third of the dequantisation (the kernel ran with its SIMDs ~75 % busy issuing)
struct Q4Raw {
  int4 q;
  uint2 m;  // (d*sc, -dmin*m) as f16 pairs of sub-blocks 2g (low nibbles) and 2g + 1 (high)
};
// Q6_K likewise: the chunk's two scales arrive as one f16 pair (d * sc_lo, d * sc_hi), and its
// 2-bit high fields as two dwords already in place for the bit assembly (tile16 layout: bmm.hip):
// 6.5 VALU per quant dword instead of 9, no per-chunk scale conversion, one scale load not three
struct Q6Raw {
  int4 l;
  uint2 x;     // high fields of quant dwords (0, 1) and (2, 3)
  unsigned s;  // (d * sc_lo, d * sc_hi) f16 pair
};
template <int T> struct BRaw { using type = WRaw<T>; };
template <> struct BRaw<T_Q4_K> { using type = Q4Raw; };
template <> struct BRaw<T_Q6_K> { using type = Q6Raw; };
// Q5_K: as Q4_K plus the chunk's high bits
struct Q5Raw {
  int4 q, h;
  uint2 m;
};
template <> struct BRaw<T_Q5_K> { using type = Q5Raw; };
// Q2_K / Q3_K: one 16-byte record per lane and chunk holds everything (tile16 layout: bmm.hip) -
// two dwords of 2-bit fields, then Q2_K's two (d*sc, -dmin*m) f16 pairs or Q3_K's dword of high
// bits and its (d*sc_lo, d*sc_hi) f16 pair
struct K23TRaw {
  int4 v;
};
template <> struct BRaw<T_Q2_K> { using type = K23TRaw; };
template <> struct BRaw<T_Q3_K> { using type = K23TRaw; };
// IQ4_XS (and IQ4_NL in the same step format): the chunk's 16 bytes of codebook indices and its
// scale d * (ls - 32) (IQ4_NL: d) pre-decoded as one f16
struct IQ4TRaw {
  int4 q;
  unsigned s;
};
template <> struct BRaw<T_IQ4_XS> { using type = IQ4TRaw; };
template <int T> using BRawT = typename BRaw<T>::type;

// chunk c of one row (raw loads in WRaw) -> the four A fragments
template <int T>
__device__ __forceinline__ void dequant_frags(const BRawT<T>& w, int c, HFrag& F) {
  const int j = c & 7;
  if constexpr (T == T_Q4_K) {
    const h2_t pa = as_h2(w.m.x), pb = as_h2(w.m.y);
    const h2_t alo = {pa[0], pa[0]}, mlo = {pa[1], pa[1]};
    const h2_t ahi = {pb[0], pb[0]}, mhi = {pb[1], pb[1]};
    const h2_t bias = {(_Float16)1024.f, (_Float16)1024.f};
    const int qv[4] = {w.q.x, w.q.y, w.q.z, w.q.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned lo = (unsigned)qv[i] & 0x0F0F0F0Fu, hi = ((unsigned)qv[i] >> 4) & 0x0F0F0F0Fu;
      F.w[4 * i + 0] = deq_pair(bytes02(lo), bias, alo, mlo);
      F.w[4 * i + 1] = deq_pair(bytes13(lo), bias, alo, mlo);
      F.w[4 * i + 2] = deq_pair(bytes02(hi), bias, ahi, mhi);
      F.w[4 * i + 3] = deq_pair(bytes13(hi), bias, ahi, mhi);
    }
    (void)j;
  } else if constexpr (T == T_Q5_K) {
    const int g = j >> 1;
    const h2_t pa = as_h2(w.m.x), pb = as_h2(w.m.y);  // pre-decoded, as for Q4_K
    const h2_t alo = {pa[0], pa[0]}, mlo = {pa[1], pa[1]};
    const h2_t ahi = {pb[0], pb[0]}, mhi = {pb[1], pb[1]};
    const h2_t bias = {(_Float16)1024.f, (_Float16)1024.f};
    const int qv[4] = {w.q.x, w.q.y, w.q.z, w.q.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      unsigned lo, hi;  // the dword's 4 low-nibble and 4 high-nibble values as bytes
      if constexpr (T == T_Q4_K) {
        lo = (unsigned)qv[i] & 0x0F0F0F0Fu;
        hi = ((unsigned)qv[i] >> 4) & 0x0F0F0F0Fu;
      } else {
        const unsigned hv = (unsigned)(i == 0 ? w.h.x : i == 1 ? w.h.y : i == 2 ? w.h.z : w.h.w);
        lo = ((unsigned)qv[i] & 0x0F0F0F0Fu) | (((hv >> (2 * g)) & 0x01010101u) << 4);
        hi = (((unsigned)qv[i] >> 4) & 0x0F0F0F0Fu) | (((hv >> (2 * g + 1)) & 0x01010101u) << 4);
      }
      F.w[4 * i + 0] = deq_pair(bytes02(lo), bias, alo, mlo);
      F.w[4 * i + 1] = deq_pair(bytes13(lo), bias, alo, mlo);
      F.w[4 * i + 2] = deq_pair(bytes02(hi), bias, ahi, mhi);
      F.w[4 * i + 3] = deq_pair(bytes13(hi), bias, ahi, mhi);
    }
  } else if constexpr (T == T_Q6_K) {
    const h2_t p = as_h2(w.s);
    const h2_t alo = {p[0], p[0]}, ahi = {p[1], p[1]};
    const h2_t zero = {(_Float16)0.f, (_Float16)0.f};
    const h2_t bias = {(_Float16)1056.f, (_Float16)1056.f};  // 1024 + 32: (q - 32) exactly
    const unsigned lv[4] = {(unsigned)w.l.x, (unsigned)w.l.y, (unsigned)w.l.z, (unsigned)w.l.w};
    // per byte of x dword e: bits 5:4 / 7:6 = the low / high 16-run fields of quant dword 2e,
    // bits 1:0 / 3:2 = those of dword 2e + 1; each lands on bits 5:4 with one shift and a mask
    const unsigned xv[2] = {w.x.x, w.x.y};
    unsigned fl[4], fh[4];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      fl[2 * e] = xv[e] & 0x30303030u;
      fh[2 * e] = (xv[e] >> 2) & 0x30303030u;
      fl[2 * e + 1] = (xv[e] << 4) & 0x30303030u;
      fh[2 * e + 1] = (xv[e] << 2) & 0x30303030u;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned lo = (lv[i] & 0x0F0F0F0Fu) | fl[i];
      const unsigned hi = ((lv[i] >> 4) & 0x0F0F0F0Fu) | fh[i];
      F.w[4 * i + 0] = deq_pair(bytes02(lo), bias, alo, zero);
      F.w[4 * i + 1] = deq_pair(bytes13(lo), bias, alo, zero);
      F.w[4 * i + 2] = deq_pair(bytes02(hi), bias, ahi, zero);
      F.w[4 * i + 3] = deq_pair(bytes13(hi), bias, ahi, zero);
    }
    (void)j;
  } else if constexpr (T == T_Q2_K || T == T_Q3_K) {
    // field dword D[i >> 1] holds quant dword i of the low run at bit 2 (i & 1) of every byte and
    // of the high run at bit 4 + 2 (i & 1): one shift and one mask each
    const unsigned D[2] = {(unsigned)w.v.x, (unsigned)w.v.y};
    const h2_t pa = as_h2((unsigned)w.v.z), pb = as_h2((unsigned)w.v.w);
    h2_t alo, ahi, mlo, mhi, bias;
    if constexpr (T == T_Q2_K) {  // (d*sc, -dmin*m) of the low run, of the high run
      alo = h2_t{pa[0], pa[0]}; mlo = h2_t{pa[1], pa[1]};
      ahi = h2_t{pb[0], pb[0]}; mhi = h2_t{pb[1], pb[1]};
      bias = h2_t{(_Float16)1024.f, (_Float16)1024.f};
    } else {                      // (d*sc_lo, d*sc_hi); 1024 + 4: (q - 4) exactly
      alo = h2_t{pb[0], pb[0]}; ahi = h2_t{pb[1], pb[1]};
      mlo = mhi = h2_t{(_Float16)0.f, (_Float16)0.f};
      bias = h2_t{(_Float16)1028.f, (_Float16)1028.f};
    }
    const unsigned H = (unsigned)w.v.z;  // Q3_K: bit i of a byte = high bit of low-run dword i, bit 4 + i of the high run's
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      unsigned lo = (D[i >> 1] >> (2 * (i & 1))) & 0x03030303u;
      unsigned hi = (D[i >> 1] >> (4 + 2 * (i & 1))) & 0x03030303u;
      if constexpr (T == T_Q3_K) {  // the high bit lands on bit 2 of its byte (neighbouring bytes' bits fall outside the mask)
        constexpr int kL[4] = {2, 1, 0, 0}, kR[4] = {0, 0, 0, 1};
        lo |= ((H << kL[i]) >> kR[i]) & 0x04040404u;
        hi |= (H >> (2 + i)) & 0x04040404u;
      }
      F.w[4 * i + 0] = deq_pair(bytes02(lo), bias, alo, mlo);
      F.w[4 * i + 1] = deq_pair(bytes13(lo), bias, alo, mlo);
      F.w[4 * i + 2] = deq_pair(bytes02(hi), bias, ahi, mhi);
      F.w[4 * i + 3] = deq_pair(bytes13(hi), bias, ahi, mhi);
    }
    (void)j;
  } else if constexpr (T == T_IQ4_XS) {
    // the codebook lookup replaces the mask step: the table holds value + 128 as unsigned bytes,
    // which go under the 1024 exponent as the other types' quants do; the bias removed is then
    // 1024 + 128 = 1152 (exact in f16: 1024 + byte <= 1279 < 2048) and one multiply by the
    // chunk's scale follows (the fma with +0 rounds once, as a multiply). VALU per quant dword
    // (8 weights): lookup 13 (and, shift + and, 4 table perms, 2 x (shift, and-or), 2 merging
    // perms), 4 magic perms, 4 pk_add, 4 pk_fma = 25, 3.1 per weight against Q4_K's 15 (1.9)
    const _Float16 sc = __builtin_bit_cast(_Float16, (unsigned short)(w.s & 0xFFFF));
    const h2_t a = {sc, sc};
    const h2_t zero = {(_Float16)0.f, (_Float16)0.f};
    const h2_t bias = {(_Float16)1152.f, (_Float16)1152.f};
    const unsigned qv[4] = {(unsigned)w.q.x, (unsigned)w.q.y, (unsigned)w.q.z, (unsigned)w.q.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      unsigned lo, hi;
      iq4_lookup<0x80u>(qv[i], lo, hi);
      F.w[4 * i + 0] = deq_pair(bytes02(lo), bias, a, zero);
      F.w[4 * i + 1] = deq_pair(bytes13(lo), bias, a, zero);
      F.w[4 * i + 2] = deq_pair(bytes02(hi), bias, a, zero);
      F.w[4 * i + 3] = deq_pair(bytes13(hi), bias, a, zero);
    }
    (void)j;
  } else {  // Q8_0: signed bytes, flipped to unsigned for the magic, one scale
    static_assert(T == T_Q8_0, "dequant_frags: unsupported type");
    const float d = h2f(w.d & 0xFFFF);
    const h2_t a = {(_Float16)d, (_Float16)d};
    const h2_t zero = {(_Float16)0.f, (_Float16)0.f};
    const h2_t bias = {(_Float16)1152.f, (_Float16)1152.f};  // 1024 + 128
    const int lo4[4] = {w.a.x, w.a.y, w.a.z, w.a.w};
    const int hi4[4] = {w.b.x, w.b.y, w.b.z, w.b.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned lo = (unsigned)lo4[i] ^ 0x80808080u, hi = (unsigned)hi4[i] ^ 0x80808080u;
      F.w[4 * i + 0] = deq_pair(bytes02(lo), bias, a, zero);
      F.w[4 * i + 1] = deq_pair(bytes13(lo), bias, a, zero);
      F.w[4 * i + 2] = deq_pair(bytes02(hi), bias, a, zero);
      F.w[4 * i + 3] = deq_pair(bytes13(hi), bias, a, zero);
    }
  }
}

// element offsets (into an x row) of chunk c's low and high 16-runs
template <int T>
__device__ __forceinline__ void chunk_runs(int c, int& off_lo, int& off_hi) {
  const int sb = c >> 3, j = c & 7;
  if constexpr (T == T_Q4_K || T == T_Q5_K || T == T_Q2_K || T == T_Q3_K) {
    off_lo = sb * 256 + 64 * (j >> 1) + 16 * (j & 1);
    off_hi = off_lo + 32;
  } else if constexpr (T == T_Q6_K) {
    off_lo = sb * 256 + 128 * (j >> 2) + 16 * (j & 3);
    off_hi = off_lo + 64;
  } else {
    off_lo = 32 * c;
    off_hi = off_lo + 16;
  }
}

__host__ __device__ constexpr int t16_kernel_type(int t) {
  return (t == T_Q4_0 || t == T_Q4_1) ? T_Q4_K : (t == T_Q5_0 || t == T_Q5_1) ? T_Q5_K : t == T_IQ4_NL ? T_IQ4_XS : t;
}
__host__ __device__ constexpr int t16_step_bytes(int t) {
  const int k = t16_kernel_type(t);
  return k == T_Q2_K ? 2048 : k == T_Q3_K ? 2048 : k == T_Q4_K ? 2560 : k == T_Q5_K ? 3072 : k == T_Q6_K ? 3584
         : k == T_Q8_0 ? 4352 : k == T_IQ4_XS ? 2304 : 0;
}

// raw loads of lane l's chunk h (8s + 4h + kq) from a tile16 step block (NT: the quant
// bytes non-temporal - decode reads every weight once; the prefill GEMM's token blocks
// re-read them, so it loads them plainly)
template <int T, bool NT = true>
__device__ __forceinline__ int4 ld_q16(const uint8_t* p) {
  if constexpr (NT) return ld_nt16(p);
  else return *reinterpret_cast<const int4*>(p);
}
template <int T, bool NT = true>
__device__ __forceinline__ void tload(BRawT<T>& w, const uint8_t* blk, int h, int l, int r16, int kq) {
  if constexpr (T == T_Q4_K) {
    w.q = ld_q16<T, NT>(blk + h * 1024 + l * 16);
    // chunk 4h + kq covers sub-blocks 2g, 2g + 1 with g = 2h + kq / 2
    w.m = *reinterpret_cast<const uint2*>(blk + 2048 + r16 * 32 + 8 * (2 * h + (kq >> 1)));
  } else if constexpr (T == T_Q5_K) {
    w.q = ld_q16<T, NT>(blk + h * 1024 + l * 16);
    w.h = *reinterpret_cast<const int4*>(blk + 2048 + r16 * 32 + 16 * (kq & 1));
    w.m = *reinterpret_cast<const uint2*>(blk + 2560 + r16 * 32 + 8 * (2 * h + (kq >> 1)));
  } else if constexpr (T == T_Q6_K) {
    w.l = ld_q16<T, NT>(blk + h * 1024 + l * 16);
    w.x = *reinterpret_cast<const uint2*>(blk + 2048 + h * 512 + l * 8);
    w.s = *reinterpret_cast<const unsigned*>(blk + 3072 + r16 * 32 + (4 * h + kq) * 4);
  } else if constexpr (T == T_Q2_K || T == T_Q3_K) {
    w.v = ld_q16<T, NT>(blk + h * 1024 + l * 16);
  } else if constexpr (T == T_IQ4_XS) {
    w.q = ld_q16<T, NT>(blk + h * 1024 + l * 16);
    w.s = *reinterpret_cast<const unsigned short*>(blk + 2048 + r16 * 16 + (4 * h + kq) * 2);
  } else {
    static_assert(T == T_Q8_0, "tload: unsupported type");
    w.a = ld_q16<T, NT>(blk + h * 2048 + l * 16);
    w.b = ld_q16<T, NT>(blk + h * 2048 + 1024 + l * 16);
    w.d = *reinterpret_cast<const unsigned short*>(blk + 4096 + h * 128 + l * 2);
  }
}

// tload through a buffer resource over the matrix (IL kernels): the step's byte offset is a
// uniform scalar (soffset), the lane's part a constant voffset and the plane offsets immediates -
// no per-step 64-bit address arithmetic, whose temporaries the register allocator placed in the
// registers of loads still in flight (a vmcnt wait on them drained the ring at every round)
typedef int v4i_t __attribute__((ext_vector_type(4)));
typedef int v2i_t __attribute__((ext_vector_type(2)));
template <int T, bool NTQ = true>
__device__ __forceinline__ void tload_rs(BRawT<T>& w, __amdgpu_buffer_rsrc_t rs, int so, int h, int l, int r16, int kq) {
  auto b128 = [&](int vo, int imm) {  // quant planes: non-temporal (aux 2: each weight is read once per step)
    const v4i_t t = __builtin_bit_cast(v4i_t, __builtin_amdgcn_raw_buffer_load_b128(rs, vo, so + imm, NTQ ? 2 : 0));
    return make_int4(t.x, t.y, t.z, t.w);
  };
  auto b128c = [&](int vo, int imm) {
    const v4i_t t = __builtin_bit_cast(v4i_t, __builtin_amdgcn_raw_buffer_load_b128(rs, vo, so + imm, 0));
    return make_int4(t.x, t.y, t.z, t.w);
  };
  auto b64 = [&](int vo, int imm) {
    const v2i_t t = __builtin_bit_cast(v2i_t, __builtin_amdgcn_raw_buffer_load_b64(rs, vo, so + imm, 0));
    return make_uint2((unsigned)t.x, (unsigned)t.y);
  };
  if constexpr (T == T_Q4_K) {
    w.q = b128(l * 16, h * 1024);
    w.m = b64(r16 * 32 + 8 * (kq >> 1), 2048 + 16 * h);
  } else if constexpr (T == T_Q5_K) {
    w.q = b128(l * 16, h * 1024);
    w.h = b128c(r16 * 32 + 16 * (kq & 1), 2048);
    w.m = b64(r16 * 32 + 8 * (kq >> 1), 2560 + 16 * h);
  } else if constexpr (T == T_Q6_K) {
    w.l = b128(l * 16, h * 1024);
    w.x = b64(l * 8, 2048 + h * 512);
    w.s = __builtin_amdgcn_raw_buffer_load_b32(rs, r16 * 32 + kq * 4, so + 3072 + 16 * h, 0);
  } else if constexpr (T == T_Q2_K || T == T_Q3_K) {
    w.v = b128(l * 16, h * 1024);
  } else if constexpr (T == T_IQ4_XS) {
    w.q = b128(l * 16, h * 1024);
    w.s = __builtin_amdgcn_raw_buffer_load_b16(rs, r16 * 16 + kq * 2, so + 2048 + 8 * h, 0);
  } else {
    static_assert(T == T_Q8_0, "tload_rs: unsupported type");
    w.a = b128(l * 16, h * 2048);
    w.b = b128(l * 16, h * 2048 + 1024);
    w.d = __builtin_amdgcn_raw_buffer_load_b16(rs, l * 2, so + 4096 + h * 128, 0);
  }
}

// Block barrier for LDS hand-offs only: waits for this wave's LDS operations, not for its
// global loads. __syncthreads() is a workgroup release/acquire, which makes every wave drain
// its outstanding global loads (s_waitcnt vmcnt(0)) - at every tile boundary that emptied
// the weight ring the loop keeps in flight across tiles.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Staged X rows are 128 halves (no pad) with their 16-B units XOR-swizzled by the token's row in
// its 16-row group (unit u of row r at u ^ (r & 15)): ds_read_b128 serves a wave in lane groups
// {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ... - two kq values x 8 token rows per group - and
// no uniform pitch keeps those 16 lanes apart (136 halves: 2-way, measured 2.1 conflict cycles
// per LDS instruction); the swizzle makes them conflict-free for the Q4_K / Q5_K / Q6_K runs
// (Q8_0's stay 2-way).
static constexpr int kT16Pitch = 128;

}  // namespace lfk
