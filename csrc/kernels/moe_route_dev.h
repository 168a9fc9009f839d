// MoE routing finish shared by moe.hip's router kernel and the routed SwiGLU GEMV (gemv.hip):
// one wave turns the per-wave partial router sums into logits, softmax, top-k (lowest index on
// ties) and renormalised weights. Both callers reduce in the same order (per-thread float4
// partials -> wave_sum_fast -> waves 0..NW-1 in order), so their routing is bit-identical.
#pragma once
#include "qdot.h"

namespace lfk {

// One thread's share of the router sums over its float4 of x: the sum of squares, and the product
// of the normalised input n = x * w_norm with a router row. Spelled with fmaf: left to
// -ffp-contract=fast, which product of a sum becomes an fma's addend is the compiler's choice per
// call site, and the two callers' logits differed in their last bits
// (tests/test_decode_fused_gpu.py::test_routed_gate_up). The callers' own sums (moe.hip's
// `ss +=` / `acc[e] +=` over the d / 4096 passes) must stay OUTSIDE these helpers, as plain adds of
// a helper's result: an add written next to a product would be fused again, per site. This moved
// every user of moe_router_fused_kernel by a few ulp - the single-row router and the batched rows
// (moe_router_rows) alike.
__device__ __forceinline__ float route_ss4(float4 x) {
  return fmaf(x.w, x.w, fmaf(x.z, x.z, fmaf(x.y, x.y, x.x * x.x)));
}
__device__ __forceinline__ float route_dot4(float4 n, float4 r) {
  return fmaf(n.w, r.w, fmaf(n.z, r.z, fmaf(n.y, r.y, n.x * r.x)));
}

// red[w][e] (e < EM): wave w's router partial of expert e; red[w][EM]: its sum of squares.
// Lane j < k returns (id_j, w_j / sum of the k picks); lane e < E returns its logit in *logit.
template <int EM, int NW>
__device__ __forceinline__ void moe_route_finish(const float (*red)[EM + 1], int E, int k, int d, float eps, int lane,
                                                 int& my_id, float& my_w, float& sel_sum, float& logit) {
  float tot = 0.f;
#pragma unroll
  for (int w = 0; w < NW; ++w) tot += red[w][EM];
  const float sc = rsqrtf(tot / (float)d + eps);
  float v = -INFINITY;
  if (lane < E) {
    float sum = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) sum += red[w][lane];
    v = sum * sc;
  }
  logit = v;
  const float m = wave_max(v);
  float p = lane < E ? __expf(v - m) : 0.f;
  p /= wave_sum(p);
  float taken = lane < E ? p : -1.f;
  sel_sum = 0.f;
  my_w = 0.f;
  my_id = 0;
  for (int j = 0; j < k; ++j) {
    float best = taken;
    int bi = lane;
    for (int o = 32; o > 0; o >>= 1) {
      const float ob = __shfl_xor(best, o);
      const int oi = __shfl_xor(bi, o);
      if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (lane == j) { my_id = bi; my_w = best; }
    sel_sum += best;
    if (lane == bi) taken = -1.f;
  }
}

}  // namespace lfk
