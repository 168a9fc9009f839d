// What the two scoring heads share (score.hip: the tile16 copy; score_w16.hip: a row-major 16-bit
// head): the running (max, rescaled sum, target, best) of a token, its merge, and the finish launch.
#pragma once
#include "kernels.h"

namespace lfk {

// Every merge is (max, rescaled sum): no logit is ever exponentiated without its maximum subtracted.
struct ScoreRun {
  float m, s, tl, bv;  // max, sum exp(l - m), the target's logit (-inf: not seen), the best logit
  int bi;              // ... and its id (lowest on ties)
};
__device__ __forceinline__ ScoreRun score_empty() {
  return ScoreRun{-__builtin_inff(), 0.f, -__builtin_inff(), -__builtin_inff(), 0x7FFFFFFF};
}
__device__ __forceinline__ void score_merge(ScoreRun& a, const ScoreRun& b) {
  const float M = fmaxf(a.m, b.m);
  if (M > -__builtin_inff()) a.s = a.s * expf(a.m - M) + b.s * expf(b.m - M);  // (exp(-inf) = 0: an empty side)
  a.m = M;
  a.tl = fmaxf(a.tl, b.tl);  // one side at most holds the target's row
  if (b.bv > a.bv || (b.bv == a.bv && b.bi < a.bi)) {
    a.bv = b.bv;
    a.bi = b.bi;
  }
}
__device__ __forceinline__ ScoreRun score_shfl_xor(const ScoreRun& r, int off) {
  return ScoreRun{__shfl_xor(r.m, off), __shfl_xor(r.s, off), __shfl_xor(r.tl, off), __shfl_xor(r.bv, off),
                  __shfl_xor(r.bi, off)};
}

// stage 2 (score.hip): a.part[range][t] over `nranges` ranges -> a.rec[t], one wave per token, the
// ranges merged in a fixed order
void score_finish(const ScoreHeadArgs& a, int nranges, hipStream_t s);

}  // namespace lfk
