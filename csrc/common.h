// Shared definitions for the MI355X (gfx950) runtime and kernels.
//
// Weight layout on the GPU ("row-planar" repack, done once at load time):
// every quantised matrix with R rows (output features) and K columns is split
// into per-field planes so each plane row is contiguous and 16-B aligned - the
// GGUF block layout (Q6_K 210 B, Q8_0 34 B) is not, which would break wide
// coalesced loads (SURVEY §2.3 "Row bytes are 16-B aligned ... blocks are not").
//
//   Q4_K : qs[R][K/256][128] | meta[R][K/256][16]   (meta = d, dmin, scales[12])
//   Q5_K : qs[R][K/256][128] | qh[R][K/256][32] | meta[R][K/256][16]
//   Q6_K : ql[R][K/256][128] | qh[R][K/256][64] | sc[R][K/256][16] | d[R][K/256] (f16)
//   Q8_0 : qs[R][K/32][32]   | d[R][K/32] (f16)
//   Q4_0 : qs[R][K/32][16]   | d[R][K/32] (f16)
//   Q4_1 : qs[R][K/32][16]   | dm[R][K/32][2] (f16 d, m)
//   Q5_0 : qs[R][K/32][16]   | qh[R][K/32] (u32) | d[R][K/32] (f16)
//   Q5_1 : qs[R][K/32][16]   | qh[R][K/32] (u32) | dm[R][K/32][2] (f16 d, m)
//          (legacy 32-weight blocks: byte j of a block's qs holds weight j in its low
//           nibble and weight j + 16 in its high nibble; bit j of qh is weight j's 5th bit)
//   Q2_K : qs[R][K/256][64]  | sc[R][K/256][16] | dm[R][K/256][2] (f16 d, dmin)
//   Q3_K : qs[R][K/256][64]  | hmask[R][K/256][32] | sc[R][K/256][12] | d[R][K/256] (f16)
//          (2- and 3-bit K-quants: the fields keep their GGUF byte order. Byte 32n + l of a
//           block's qs holds the low two bits of weights 128n + 32j + l, j = 0..3, at bit 2j; bit
//           4n + j of hmask[l] is Q3_K's third bit of the same weight; sc holds Q2_K's sixteen
//           (scale | min << 4) bytes or Q3_K's sixteen packed 6-bit scales. Q3_K's 12-byte scale
//           rows are 4-byte aligned, and its sc / d planes start 16-byte aligned when R * K / 256
//           is a multiple of 4 (4-byte aligned otherwise): they are read as dwords / halves.)
//   IQ4_NL : qs[R][K/32][16]  | d[R][K/32] (f16)                     (Q4_0's layout)
//   IQ4_XS : qs[R][K/256][128] | sc[R][K/256][8]
//          (the non-linear 4-bit pair: a nibble indexes the 16-entry int8 codebook kIQ4Values.
//           Every 32-weight chunk is contiguous with Q4_0's nibble order - byte j of chunk c's 16
//           holds weight 32c + j low and weight 32c + 16 + j high. IQ4_XS's sc keeps the GGUF
//           fields as they stand: f16 d | u16 scales_h | u8 scales_l[4], one aligned 8-byte load
//           per superblock; sub-block ib has the 6-bit scale ls = low nibble ib of scales_l |
//           bit pair ib of scales_h << 4 and the weight is d * (ls - 32) * codebook[nibble].)
//   F16 / F32 : [R][K] unchanged
//
// Total bytes are identical to the GGUF tensor (no padding), so 4.6 GB of
// Llama-3-8B Q4_K_M weights stay 4.6 GB on HBM.
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>

namespace lfk {

enum QType : int {
  T_F32 = 0,
  T_F16 = 1,
  T_Q4_0 = 2,
  T_Q4_1 = 3,
  T_Q5_0 = 6,
  T_Q5_1 = 7,
  T_Q8_0 = 8,
  T_Q2_K = 10,
  T_Q3_K = 11,
  T_Q4_K = 12,
  T_Q5_K = 13,
  T_Q6_K = 14,
  T_IQ4_NL = 20,
  T_IQ4_XS = 23,
  T_BF16 = 30,
};

struct TypeInfo {
  int block;   // weights per block
  int bytes;   // bytes per block
};

inline TypeInfo type_info(int t) {
  switch (t) {
    case T_F32: return {1, 4};
    case T_F16: return {1, 2};
    case T_BF16: return {1, 2};
    case T_Q4_0: return {32, 18};
    case T_Q4_1: return {32, 20};
    case T_Q5_0: return {32, 22};
    case T_Q5_1: return {32, 24};
    case T_Q8_0: return {32, 34};
    case T_Q2_K: return {256, 84};
    case T_Q3_K: return {256, 110};
    case T_Q4_K: return {256, 144};
    case T_Q5_K: return {256, 176};
    case T_Q6_K: return {256, 210};
    case T_IQ4_NL: return {32, 18};
    case T_IQ4_XS: return {256, 136};
  }
  throw std::runtime_error("unsupported ggml type " + std::to_string(t));
}

// the non-linear 4-bit codebook shared by IQ4_NL and IQ4_XS
constexpr int8_t kIQ4Values[16] = {-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113};

inline bool is_legacy_block_type(int t) { return t == T_Q4_0 || t == T_Q4_1 || t == T_Q5_0 || t == T_Q5_1; }

// MoE expert tensors of the legacy 32-weight block types are not supported (attention, router
// and embeddings of such a file are): refuse the model at load, naming the tensor.
// The same holds for the 2- and 3-bit K-quants Q2_K and Q3_K and for IQ4_NL and IQ4_XS.
inline void check_expert_type(const std::string& tensor, int t) {
  if (!is_legacy_block_type(t) && t != T_Q2_K && t != T_Q3_K && t != T_IQ4_NL && t != T_IQ4_XS) return;
  const char* n = t == T_Q4_0 ? "Q4_0" : t == T_Q4_1 ? "Q4_1" : t == T_Q5_0 ? "Q5_0" : t == T_Q5_1 ? "Q5_1"
                  : t == T_Q2_K ? "Q2_K" : t == T_Q3_K ? "Q3_K" : t == T_IQ4_NL ? "IQ4_NL" : "IQ4_XS";
  throw std::runtime_error("unsupported expert tensor " + tensor + ": type " + n +
                           " (MoE experts must be Q4_K, Q5_K, Q6_K, Q8_0, F16 or F32)");
}

inline size_t qbytes(int t, size_t rows, size_t K) {
  TypeInfo ti = type_info(t);
  if (K % ti.block) throw std::runtime_error("qbytes: K must be a multiple of the type's block size");
  return rows * (K / ti.block) * ti.bytes;
}

// Plane offsets (bytes from the matrix base) for the planar layout. Usable on host and device.
struct Planes {
  size_t p0, p1, p2, p3;  // start of plane 0..3
  size_t s0, s1, s2, s3;  // per-row stride of plane 0..3
};

#if defined(__HIPCC__)
#define LFK_HD __host__ __device__ __forceinline__
#else
#define LFK_HD inline
#endif

LFK_HD Planes planes_of(int t, size_t R, size_t K) {
  Planes p{0, 0, 0, 0, 0, 0, 0, 0};
  size_t nsb = K / 256, nb = K / 32;
  switch (t) {
    case T_Q4_K:
      p.s0 = nsb * 128; p.s1 = nsb * 16;
      p.p0 = 0; p.p1 = R * p.s0;
      break;
    case T_Q5_K:
      p.s0 = nsb * 128; p.s1 = nsb * 32; p.s2 = nsb * 16;
      p.p0 = 0; p.p1 = R * p.s0; p.p2 = p.p1 + R * p.s1;
      break;
    case T_Q6_K:
      p.s0 = nsb * 128; p.s1 = nsb * 64; p.s2 = nsb * 16; p.s3 = nsb * 2;
      p.p0 = 0; p.p1 = R * p.s0; p.p2 = p.p1 + R * p.s1; p.p3 = p.p2 + R * p.s2;
      break;
    case T_Q2_K:
      p.s0 = nsb * 64; p.s1 = nsb * 16; p.s2 = nsb * 4;
      p.p0 = 0; p.p1 = R * p.s0; p.p2 = p.p1 + R * p.s1;
      break;
    case T_Q3_K:
      p.s0 = nsb * 64; p.s1 = nsb * 32; p.s2 = nsb * 12; p.s3 = nsb * 2;
      p.p0 = 0; p.p1 = R * p.s0; p.p2 = p.p1 + R * p.s1; p.p3 = p.p2 + R * p.s2;
      break;
    case T_Q8_0:
      p.s0 = nb * 32; p.s1 = nb * 2;
      p.p0 = 0; p.p1 = R * p.s0;
      break;
    case T_IQ4_XS:
      p.s0 = nsb * 128; p.s1 = nsb * 8;
      p.p0 = 0; p.p1 = R * p.s0;
      break;
    case T_Q4_0: case T_Q4_1: case T_IQ4_NL:
      p.s0 = nb * 16; p.s1 = nb * (t == T_Q4_1 ? 4 : 2);
      p.p0 = 0; p.p1 = R * p.s0;
      break;
    case T_Q5_0: case T_Q5_1:
      p.s0 = nb * 16; p.s1 = nb * 4; p.s2 = nb * (t == T_Q5_0 ? 2 : 4);
      p.p0 = 0; p.p1 = R * p.s0; p.p2 = p.p1 + R * p.s1;
      break;
    case T_F16: case T_BF16:
      p.s0 = K * 2; break;
    case T_F32:
      p.s0 = K * 4; break;
    default: break;
  }
  return p;
}

}  // namespace lfk
