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
  const TypeLayout L = type_layout(type);
  if (!L.nfields) throw std::runtime_error("repack: unsupported type");
  const size_t start[4] = {P.p0, P.p1, P.p2, P.p3}, stride[4] = {P.s0, P.s1, P.s2, P.s3};
#pragma omp parallel for schedule(static)
  for (long long ii = 0; ii < (long long)R; ++ii) {
    const size_t i = (size_t)ii;
    const size_t dr = G > 0 ? (i / G) * 2 * G + off + i % G : off + i;
    const uint8_t* srow = src + ((r0 + (neox_hd ? neox_src_row(i, neox_hd) : i)) * nb_src + b0) * ti.bytes;
    if (L.nfields == 1) {  // one plane (F16 / BF16 / F32): the row is contiguous on both sides
      std::memcpy(dst + dr * stride[0], srow, stride[0]);
      continue;
    }
    for (int f = 0; f < L.nfields; ++f) {  // field f of every block of the row -> plane f
      const size_t n = (size_t)L.f[f].bytes;
      const uint8_t* s = srow + L.f[f].src;
      uint8_t* d = dst + start[f] + dr * stride[f];
      for (size_t b = 0; b < nb; ++b) std::memcpy(d + b * n, s + b * ti.bytes, n);
    }
  }
}

}  // namespace lfk
