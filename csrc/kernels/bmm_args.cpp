// The BmmArgs of a batched decode layer's projections (kernels.h), host code only: the one place
// where a projection form's descriptor is assembled, for the engine and for the test bindings.
#include <algorithm>

#include "kernels.h"

namespace lfk {

void bmm_fold_norm(BmmArgs& a, const BmmNorm& norm) {
  if (!norm.xf) return;
  a.xf = norm.xf; a.ldxf = norm.ldxf; a.norm_w = norm.norm_w; a.eps = norm.eps;
}

BmmArgs bmm_qkv_sk_args(const QMat m[3], const BmmNorm& norm, int B, float* out, int ldo, float* ss_out,
                        const int* pos, const float2* rope, int head_dim, int n_ctx) {
  BmmArgs a;
  a.w = m[0]; a.n_out = m[0].rows; a.out = out; a.ldo = ldo; a.B = B;
  a.nseg = 3;
  a.seg_base[1] = m[1].base; a.seg_rows[1] = m[1].rows; a.seg_out[1] = out + m[0].rows;
  a.seg_base[2] = m[2].base; a.seg_rows[2] = m[2].rows; a.seg_out[2] = out + m[0].rows + m[1].rows;
  // runs of equal tile16 format (Q4_0 / Q4_1 copies are in the Q4_K format, Q5_0 / Q5_1 in Q5_K's)
  const int tq = t16_format(m[0].type), tk = t16_format(m[1].type), tv = t16_format(m[2].type);
  a.seg_split = tk != tq ? 1 : tv != tq ? 2 : 3;
  a.type2 = tk != tq ? tk : tv != tq ? tv : 0;
  a.qkv_sk = true;
  a.qkv.pos = pos; a.qkv.rope = rope; a.qkv.head_dim = head_dim; a.qkv.n_ctx = n_ctx;
  bmm_fold_norm(a, norm);
  a.ss_out = ss_out;
  return a;
}

std::vector<BmmArgs> bmm_qkv_runs(const QMat* m, int n, const __half* xh, int ldh, const BmmNorm& norm, int B,
                                  float* out, int ldo, const BmmArgs::Qkv* epi, const float* bias) {
  int off[3] = {0, 0, 0};  // first column of each matrix's rows in an out / bias row
  for (int i = 0; i + 1 < n; ++i) off[i + 1] = off[i] + m[i].rows;
  std::vector<BmmArgs> rl;
  for (int i = 0; i < n;) {
    int j = i + 1;
    while (j < n && t16_format(m[j].type) == t16_format(m[i].type)) ++j;
    for (int b0 = 0; b0 < B; b0 += kBmmMaxRows) {
      BmmArgs a;
      a.w = m[i]; a.xh = xh + (size_t)b0 * ldh; a.ldh = ldh;
      a.out = out + off[i] + (size_t)b0 * ldo; a.ldo = ldo; a.n_out = m[i].rows;
      a.B = std::min(kBmmMaxRows, B - b0);
      a.nseg = j - i;
      for (int k = 1; k < a.nseg; ++k) {
        a.seg_base[k] = m[i + k].base; a.seg_rows[k] = m[i + k].rows;
        a.seg_out[k] = out + off[i + k] + (size_t)b0 * ldo;
      }
      if (norm.xf) {
        BmmNorm g = norm;
        g.xf += (size_t)b0 * norm.ldxf;
        bmm_fold_norm(a, g);
      }
      if (epi) {
        a.qkv_epi = true;
        a.qkv = *epi;
        a.qkv.q_out += (size_t)b0 * epi->q_ld; a.qkv.pos += b0; a.qkv.slots += b0;
        for (int k = 0; k < a.nseg; ++k) {
          a.qkv.kind[k] = i + k;
          a.qkv.bias[k] = bias ? bias + off[i + k] : nullptr;
        }
      }
      rl.push_back(a);
    }
    i = j;
  }
  return rl;
}

bool bmm_launch_runs(const std::vector<BmmArgs>& runs, bool try_two, hipStream_t s) {
  // bumped layers (Q|K Q4_K + V Q6_K): both runs in one launch
  const bool one = try_two && runs.size() == 2 && bmm_qkv2_supported(runs[0], runs[1]);
  if (one) bmm_qkv2(runs[0], runs[1], s);
  else
    for (const BmmArgs& a : runs) bmm(a, s);
  return one;
}

BmmArgs bmm_proj_args(const QMat& w, const __half* xh, int ldh, float* out, int ldo, int B) {
  BmmArgs a;
  a.w = w; a.xh = xh; a.ldh = ldh; a.out = out; a.ldo = ldo; a.n_out = w.rows; a.B = B;
  return a;
}

BmmArgs bmm_gate_up_args(const QMat& w, const __half* xh, int ldh, const BmmNorm& norm, int B, __half* h_out,
                         int ldh_out) {
  BmmArgs a = bmm_proj_args(w, xh, ldh, nullptr, 0, B);
  bmm_fold_norm(a, norm);
  a.swiglu_epi = true; a.h_out = h_out; a.ldh_out = ldh_out;
  return a;
}

BmmArgs bmm_down_args(const QMat& w, const __half* xh, int ldh, float* out, int ldo, int B, float* zero, int zero_n) {
  BmmArgs a = bmm_proj_args(w, xh, ldh, out, ldo, B);
  a.zero = zero; a.zero_n = zero ? zero_n : 0;
  return a;
}

BmmArgs bmm_moe_gate_up_args(const QMat& w, const __half* xh, int ldh, const BmmNorm& norm, int B, __half* h_out,
                             int ldh_out, const float* ew, int ew_ld, int tiles_per_expert) {
  BmmArgs a = bmm_gate_up_args(w, xh, ldh, norm, B, h_out, ldh_out);
  a.ew = ew; a.ew_ld = ew_ld; a.tiles_per_expert = tiles_per_expert;
  return a;
}

BmmArgs bmm_moe_down_args(const QMat& w, const __half* xh, int ldh, float* out, int ldo, int B, float* zero,
                          int zero_n, const float* ew, int ew_ld, int steps_per_expert) {
  BmmArgs a = bmm_down_args(w, xh, ldh, out, ldo, B, zero, zero_n);
  a.ew = ew; a.ew_ld = ew_ld; a.steps_per_expert = steps_per_expert;
  return a;
}

}  // namespace lfk
