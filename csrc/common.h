// Shared definitions for the MI355X (gfx950) runtime and kernels.
//
// Weight layout on the GPU ("row-planar" repack, done once at load time):
// every quantised matrix with R rows (output features) and K columns is split
// into per-field planes so each plane row is contiguous and 16-B aligned - the
// GGUF block layout (Q6_K 210 B, Q8_0 34 B) is not, which would break wide
// coalesced loads (SURVEY §2.3 "Row bytes are 16-B aligned ... blocks are not").
// type_layout() below is the authority on which GGUF bytes form which plane; this comment says
// what the planes hold (nibble order, alignment), which the table does not.
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

// ---------------------------------------------------------------- the layout table
// One row per weight type: its name, the weights per block, and its GGUF fields in plane order,
// each as {offset inside the GGUF block, bytes}. Everything else about the planar layout follows:
// bytes per block = the sum of the field bytes, a plane's row stride = blocks per row x field
// bytes, a plane's start = the sum of R x stride over the planes before it, and the repack is one
// loop over the fields (runtime/repack.cpp). This table is the authority on offsets; the comment
// at the top of this file describes what the fields hold.
struct TypeField {
  int src, bytes;
};
struct TypeLayout {
  const char* name;
  int block;       // weights per block (0: not a weight type)
  int nfields;
  TypeField f[4];  // plane 0..3
};

constexpr TypeLayout type_layout(int t) {
  switch (t) {
    case T_Q4_K: return {"Q4_K", 256, 2, {{16, 128}, {0, 16}}};
    case T_Q5_K: return {"Q5_K", 256, 3, {{48, 128}, {16, 32}, {0, 16}}};
    case T_Q6_K: return {"Q6_K", 256, 4, {{0, 128}, {128, 64}, {192, 16}, {208, 2}}};
    case T_Q2_K: return {"Q2_K", 256, 3, {{16, 64}, {0, 16}, {80, 4}}};
    case T_Q3_K: return {"Q3_K", 256, 4, {{32, 64}, {0, 32}, {96, 12}, {108, 2}}};
    case T_IQ4_XS: return {"IQ4_XS", 256, 2, {{8, 128}, {0, 8}}};
    case T_Q8_0: return {"Q8_0", 32, 2, {{2, 32}, {0, 2}}};
    case T_Q4_0: return {"Q4_0", 32, 2, {{2, 16}, {0, 2}}};
    case T_IQ4_NL: return {"IQ4_NL", 32, 2, {{2, 16}, {0, 2}}};
    case T_Q4_1: return {"Q4_1", 32, 2, {{4, 16}, {0, 4}}};
    case T_Q5_0: return {"Q5_0", 32, 3, {{6, 16}, {2, 4}, {0, 2}}};
    case T_Q5_1: return {"Q5_1", 32, 3, {{8, 16}, {4, 4}, {0, 4}}};
    case T_F16: return {"F16", 1, 1, {{0, 2}}};
    case T_BF16: return {"BF16", 1, 1, {{0, 2}}};
    case T_F32: return {"F32", 1, 1, {{0, 4}}};
  }
  return {nullptr, 0, 0, {}};
}

// ---------------------------------------------------------------- named type lists
// LIST(X, ...) expands X(T, ...) for every type of the list. A launcher names the list it serves
// (LFK_DISPATCH below); a new type joins the lists whose kernels decode it.
//
// every type with a GPU kernel (GEMV, dequantising GEMM, embedding gather)
#define LFK_TYPES_KERNEL(X, ...)                                                                              \
  X(T_Q4_K, __VA_ARGS__) X(T_Q5_K, __VA_ARGS__) X(T_Q6_K, __VA_ARGS__) X(T_Q8_0, __VA_ARGS__)                \
  X(T_Q4_0, __VA_ARGS__) X(T_Q4_1, __VA_ARGS__) X(T_Q5_0, __VA_ARGS__) X(T_Q5_1, __VA_ARGS__)                \
  X(T_Q2_K, __VA_ARGS__) X(T_Q3_K, __VA_ARGS__) X(T_IQ4_NL, __VA_ARGS__) X(T_IQ4_XS, __VA_ARGS__)            \
  X(T_F16, __VA_ARGS__) X(T_F32, __VA_ARGS__)
// the GEMV instantiations of kernels/gemv.hip itself ...
#define LFK_TYPES_GEMV_MAIN(X, ...)                                                                           \
  X(T_Q4_K, __VA_ARGS__) X(T_Q5_K, __VA_ARGS__) X(T_Q6_K, __VA_ARGS__) X(T_Q8_0, __VA_ARGS__)                \
  X(T_F16, __VA_ARGS__) X(T_F32, __VA_ARGS__)
// ... and those of kernels/gemv_legacy.hip (a second translation unit, for compile time)
#define LFK_TYPES_GEMV_LEGACY(X, ...)                                                                         \
  X(T_Q4_0, __VA_ARGS__) X(T_Q4_1, __VA_ARGS__) X(T_Q5_0, __VA_ARGS__) X(T_Q5_1, __VA_ARGS__)                \
  X(T_Q2_K, __VA_ARGS__) X(T_Q3_K, __VA_ARGS__) X(T_IQ4_NL, __VA_ARGS__) X(T_IQ4_XS, __VA_ARGS__)
// MoE expert tensors (the down GEMV's types)
#define LFK_TYPES_MOE(X, ...)                                                                                 \
  X(T_Q4_K, __VA_ARGS__) X(T_Q5_K, __VA_ARGS__) X(T_Q6_K, __VA_ARGS__) X(T_Q8_0, __VA_ARGS__)                \
  X(T_F16, __VA_ARGS__) X(T_F32, __VA_ARGS__)
// the tile16 kernel formats (kernels/bmm.hip; the other quantised types are repacked into one of these)
#define LFK_TYPES_T16(X, ...)                                                                                 \
  X(T_Q4_K, __VA_ARGS__) X(T_Q5_K, __VA_ARGS__) X(T_Q6_K, __VA_ARGS__) X(T_Q8_0, __VA_ARGS__)                \
  X(T_Q2_K, __VA_ARGS__) X(T_Q3_K, __VA_ARGS__) X(T_IQ4_XS, __VA_ARGS__)
// the quantised types: sources of the tile16 repack, and the AVX2 CPU GEMM
#define LFK_TYPES_QUANT(X, ...)                                                                               \
  X(T_Q4_K, __VA_ARGS__) X(T_Q5_K, __VA_ARGS__) X(T_Q6_K, __VA_ARGS__) X(T_Q8_0, __VA_ARGS__)                \
  X(T_Q4_0, __VA_ARGS__) X(T_Q4_1, __VA_ARGS__) X(T_Q5_0, __VA_ARGS__) X(T_Q5_1, __VA_ARGS__)                \
  X(T_Q2_K, __VA_ARGS__) X(T_Q3_K, __VA_ARGS__) X(T_IQ4_NL, __VA_ARGS__) X(T_IQ4_XS, __VA_ARGS__)

// LFK_DISPATCH(LIST, t, otherwise, body): run `body` with QT = the runtime type t as a constant
// when t is in LIST, else `otherwise` (a throw, a call of the next launcher, or nothing).
// LFK_TYPE_IN(LIST, t): whether t is in LIST (t is evaluated once per type of the list).
#define LFK_DISPATCH_CASE_(T, ...) case T: { constexpr int QT = T; __VA_ARGS__; } break;
#define LFK_DISPATCH(LIST, t, otherwise, ...)                \
  switch (t) {                                               \
    LIST(LFK_DISPATCH_CASE_, __VA_ARGS__)                    \
    default: { otherwise; } break;                           \
  }
#define LFK_TYPE_IS_(T, t) || (t) == T
#define LFK_TYPE_IN(LIST, t) (false LIST(LFK_TYPE_IS_, t))

// whether a launcher that dispatches over LFK_TYPES_KERNEL serves t
inline bool dispatchable_type(int t) { return LFK_TYPE_IN(LFK_TYPES_KERNEL, t); }

struct TypeInfo {
  int block;   // weights per block
  int bytes;   // bytes per block
};

inline TypeInfo type_info(int t) {
  const TypeLayout L = type_layout(t);
  if (!L.block) throw std::runtime_error("unsupported ggml type " + std::to_string(t));
  TypeInfo ti{L.block, 0};
  for (int i = 0; i < L.nfields; ++i) ti.bytes += L.f[i].bytes;
  return ti;
}

// the non-linear 4-bit codebook shared by IQ4_NL and IQ4_XS
constexpr int8_t kIQ4Values[16] = {-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113};

// MoE expert tensors of the kernel types outside LFK_TYPES_MOE are not supported (attention, router
// and embeddings of such a file are): refuse the model at load, naming the tensor. These are the
// legacy 32-weight block types, the 2- and 3-bit K-quants Q2_K and Q3_K, and IQ4_NL and IQ4_XS.
inline void check_expert_type(const std::string& tensor, int t) {
  if (!LFK_TYPE_IN(LFK_TYPES_KERNEL, t) || LFK_TYPE_IN(LFK_TYPES_MOE, t)) return;
  throw std::runtime_error("unsupported expert tensor " + tensor + ": type " + type_layout(t).name +
                           " (MoE experts must be Q4_K, Q5_K, Q6_K, Q8_0, F16 or F32)");
}

inline size_t qbytes(int t, size_t rows, size_t K) {
  TypeInfo ti = type_info(t);
  if (K % ti.block) throw std::runtime_error("qbytes: K must be a multiple of the type's block size");
  return rows * (K / ti.block) * ti.bytes;
}

// Plane offsets (bytes from the matrix base) for the planar layout, computed on the host and
// handed to the kernels by value.
struct Planes {
  size_t p0, p1, p2, p3;  // start of plane 0..3
  size_t s0, s1, s2, s3;  // per-row stride of plane 0..3
};

// all zero for a type outside the table, and for the planes a type does not have
inline Planes planes_of(int t, size_t R, size_t K) {
  const TypeLayout L = type_layout(t);
  size_t start[4] = {0, 0, 0, 0}, stride[4] = {0, 0, 0, 0}, at = 0;
  for (int i = 0; i < L.nfields; ++i) {
    stride[i] = K / L.block * L.f[i].bytes;
    start[i] = at;
    at += R * stride[i];
  }
  return {start[0], start[1], start[2], start[3], stride[0], stride[1], stride[2], stride[3]};
}

}  // namespace lfk
