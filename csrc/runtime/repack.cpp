#include "repack.h"

#include <cstring>
#include <stdexcept>

#include "../common.h"
#include "gguf.h"

namespace lfk {

void repack_planar(int type, const uint8_t* src, size_t K_src, size_t r0, size_t R, size_t c0, size_t K,
                   uint8_t* dst, size_t R_dst, int G, int off, size_t neox_hd) {
  const TypeInfo ti = type_info(type);
  if (K % ti.block || c0 % ti.block || K_src % ti.block) throw std::runtime_error("repack: unaligned column slice");
  const size_t nb_src = K_src / ti.block, nb = K / ti.block, b0 = c0 / ti.block;
  const Planes P = planes_of(type, R_dst, K);
  if (neox_hd && (neox_hd % 2 || r0 % neox_hd || R % neox_hd)) throw std::runtime_error("repack: NeoX rows must be whole heads");
  switch (type) {
    case T_Q4_K: case T_Q5_K: case T_Q6_K: case T_Q8_0: case T_F16: case T_BF16: case T_F32: break;
    case T_Q4_0: case T_Q4_1: case T_Q5_0: case T_Q5_1: break;
    case T_Q2_K: case T_Q3_K: break;
    case T_IQ4_NL: case T_IQ4_XS: break;
    default: throw std::runtime_error("repack: unsupported type");
  }
#pragma omp parallel for schedule(static)
  for (long long ii = 0; ii < (long long)R; ++ii) {
    const size_t i = (size_t)ii;
    const size_t dr = G > 0 ? (i / G) * 2 * G + off + i % G : off + i;
    const uint8_t* srow = src + ((r0 + (neox_hd ? neox_src_row(i, neox_hd) : i)) * nb_src + b0) * ti.bytes;
    switch (type) {
      case T_Q4_K:
        for (size_t b = 0; b < nb; ++b) {
          const uint8_t* blk = srow + b * 144;
          std::memcpy(dst + P.p1 + dr * P.s1 + b * 16, blk, 16);
          std::memcpy(dst + P.p0 + dr * P.s0 + b * 128, blk + 16, 128);
        }
        break;
      case T_Q5_K:
        for (size_t b = 0; b < nb; ++b) {
          const uint8_t* blk = srow + b * 176;
          std::memcpy(dst + P.p2 + dr * P.s2 + b * 16, blk, 16);
          std::memcpy(dst + P.p1 + dr * P.s1 + b * 32, blk + 16, 32);
          std::memcpy(dst + P.p0 + dr * P.s0 + b * 128, blk + 48, 128);
        }
        break;
      case T_Q6_K:
        for (size_t b = 0; b < nb; ++b) {
          const uint8_t* blk = srow + b * 210;
          std::memcpy(dst + P.p0 + dr * P.s0 + b * 128, blk, 128);
          std::memcpy(dst + P.p1 + dr * P.s1 + b * 64, blk + 128, 64);
          std::memcpy(dst + P.p2 + dr * P.s2 + b * 16, blk + 192, 16);
          std::memcpy(dst + P.p3 + dr * P.s3 + b * 2, blk + 208, 2);
        }
        break;
      case T_Q2_K:
        for (size_t b = 0; b < nb; ++b) {
          const uint8_t* blk = srow + b * 84;
          std::memcpy(dst + P.p1 + dr * P.s1 + b * 16, blk, 16);
          std::memcpy(dst + P.p0 + dr * P.s0 + b * 64, blk + 16, 64);
          std::memcpy(dst + P.p2 + dr * P.s2 + b * 4, blk + 80, 4);
        }
        break;
      case T_Q3_K:
        for (size_t b = 0; b < nb; ++b) {
          const uint8_t* blk = srow + b * 110;
          std::memcpy(dst + P.p1 + dr * P.s1 + b * 32, blk, 32);
          std::memcpy(dst + P.p0 + dr * P.s0 + b * 64, blk + 32, 64);
          std::memcpy(dst + P.p2 + dr * P.s2 + b * 12, blk + 96, 12);
          std::memcpy(dst + P.p3 + dr * P.s3 + b * 2, blk + 108, 2);
        }
        break;
      case T_Q8_0:
        for (size_t b = 0; b < nb; ++b) {
          const uint8_t* blk = srow + b * 34;
          std::memcpy(dst + P.p1 + dr * P.s1 + b * 2, blk, 2);
          std::memcpy(dst + P.p0 + dr * P.s0 + b * 32, blk + 2, 32);
        }
        break;
      case T_IQ4_XS:
        for (size_t b = 0; b < nb; ++b) {
          const uint8_t* blk = srow + b * 136;
          std::memcpy(dst + P.p1 + dr * P.s1 + b * 8, blk, 8);  // d | scales_h | scales_l[4]
          std::memcpy(dst + P.p0 + dr * P.s0 + b * 128, blk + 8, 128);
        }
        break;
      case T_Q4_0:
      case T_IQ4_NL:
      case T_Q4_1: {
        const size_t sc = type == T_Q4_1 ? 4 : 2;  // d, or d and m
        for (size_t b = 0; b < nb; ++b) {
          const uint8_t* blk = srow + b * ti.bytes;
          std::memcpy(dst + P.p1 + dr * P.s1 + b * sc, blk, sc);
          std::memcpy(dst + P.p0 + dr * P.s0 + b * 16, blk + sc, 16);
        }
        break;
      }
      case T_Q5_0:
      case T_Q5_1: {
        const size_t sc = type == T_Q5_0 ? 2 : 4;
        for (size_t b = 0; b < nb; ++b) {
          const uint8_t* blk = srow + b * ti.bytes;
          std::memcpy(dst + P.p2 + dr * P.s2 + b * sc, blk, sc);
          std::memcpy(dst + P.p1 + dr * P.s1 + b * 4, blk + sc, 4);
          std::memcpy(dst + P.p0 + dr * P.s0 + b * 16, blk + sc + 4, 16);
        }
        break;
      }
      case T_F16:
      case T_BF16:
        std::memcpy(dst + dr * P.s0, srow, K * 2);
        break;
      case T_F32:
        std::memcpy(dst + dr * P.s0, srow, K * 4);
        break;
      default:
        break;
    }
  }
}

}  // namespace lfk
