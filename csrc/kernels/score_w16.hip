// The scoring head on a row-major BF16 / F16 lm_head, no dequantisation (kernels.h score_head_w16):
// score_head's contract - per row lp(target), log-sum-exp, best id, lp(best), no [T][V] logits - with
// gemm_bf16w's weight path: HBM -> 16-byte loads of whole 128-byte lines -> ds_write_b128 ->
// ds_read_b128 -> MFMA, no VALU instruction on a weight.
//
// Work split. A 256-thread block (4 waves) owns TM tokens x a contiguous RANGE of 128-row vocabulary
// groups and walks (group, K) as ONE sequence of 64-deep steps: the 3-deep register ring and the LDS
// double buffer of gemm_bf16w's wide regime run across the group borders, so the loads of the next
// group's first steps are in flight while a group's last MFMAs and its reduction run.
//
// Operands. The weights are the A operand of v_mfma_f32_32x32x16_{bf16,f16} and x the B operand (the
// other way round from gemm_bf16w's wide tiles): accumulator m of wave w then holds in lane l, for
// the ONE token 32 m + (l & 31), the 16 vocabulary rows 32 w + (r & 3) + 8 (r >> 2) + 4 (l >> 5) of
// the group. A lane's tokens never change over the range, so its running (max, sum exp(l - max),
// target logit, best logit, best id) per token tile lives in registers and a group is folded into it
// in lane: no shuffle, no LDS, no barrier beyond the K loop's own. (With x as A a lane would hold one
// vocabulary row for 16 tokens: a 32-lane butterfly over five-word records for 16 MT values per
// group.) At the end of the range: one xor-32 merge in each wave, the 4 waves through LDS in wave
// order, one partial per token at part[range][t]; score_finish merges the ranges.
//
// Rows >= V are loaded clamped to row V - 1 and masked before they can enter a maximum; rows >= T
// load row T - 1 and are never stored. No split-K, no atomics: two runs are bit-equal.
#include <algorithm>
#include <stdexcept>

#include "qdot.h"
#include "score_dev.h"

namespace lfk {

typedef __attribute__((ext_vector_type(8))) __bf16 sw16_bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 sw16_f16x8;
typedef __attribute__((ext_vector_type(16))) float sw16_f32x16;

static constexpr int SW16_BK = 64, SW16_PITCH = SW16_BK + 8, SW16_GROUP = 128;  // elements; rows per group

template <bool F16, int TM>
__global__ __launch_bounds__(256) void score_head_w16_kernel(ScoreHeadArgs a, int gpr, int ngroups) {
  constexpr int BNT = SW16_GROUP, NT = 256, BK = SW16_BK, PITCH = SW16_PITCH;
  constexpr int WL = BNT * 8 / NT, XL = TM * 8 / NT, MT = TM / 32;  // 16-B loads per thread and step; token tiles
  __shared__ __attribute__((aligned(16))) unsigned short lds[2 * (TM + BNT) * PITCH];
  static_assert(sizeof(ScoreRun) * 4 * TM <= sizeof(lds), "the waves' merge fits the tile buffers");
  auto Xs = [&](int b) { return lds + b * TM * PITCH; };
  auto Ws = [&](int b) { return lds + 2 * TM * PITCH + b * BNT * PITCH; };
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 31, lh = lane >> 5;
  const int V = a.V, K = a.w.K, T = a.T, nk = K / BK;
  const int t0 = blockIdx.y * TM;
  const int g0 = blockIdx.x * gpr, g1 = min(ngroups, g0 + gpr);
  const int total = (g1 - g0) * nk;  // steps of this block, >= 1

  // this thread's 16-B units of a step: unit u = tid + NT i -> row u >> 3, k offset 8 (u & 7)
  const unsigned short* wg = reinterpret_cast<const unsigned short*>(a.w.base);
  const unsigned short* xp[XL];
#pragma unroll
  for (int i = 0; i < XL; ++i) {
    const int u = tid + NT * i;
    xp[i] = reinterpret_cast<const unsigned short*>(a.x) + (size_t)min(t0 + (u >> 3), T - 1) * K + 8 * (u & 7);
  }
  // The ring's stages are named structs (fixed VGPRs, no private memory) and every load is
  // unconditional, as in gemm_bf16w. The load cursor (lg, lk) runs 3 steps ahead of the compute
  // cursor and stops at the range's last step (clamped repeats, never stored to LDS).
  struct Stage {
    i32x4_t w[WL], x[XL];
  };
  int lg = g0, lk = 0;
  auto load_step = [&](Stage& st) {
    const int k0 = lk * BK;
#pragma unroll
    for (int i = 0; i < XL; ++i) st.x[i] = *reinterpret_cast<const i32x4_t*>(xp[i] + k0);
#pragma unroll
    for (int i = 0; i < WL; ++i) {
      const int u = tid + NT * i;
      const int row = min(lg * BNT + (u >> 3), V - 1);
      st.w[i] = *reinterpret_cast<const i32x4_t*>(wg + (size_t)row * K + 8 * (u & 7) + k0);
    }
    if (lg != g1 - 1 || lk != nk - 1) {
      if (++lk == nk) {
        lk = 0;
        ++lg;
      }
    }
  };
  auto store_step = [&](const Stage& st, int buf) {
#pragma unroll
    for (int i = 0; i < XL; ++i) {
      const int u = tid + NT * i;
      *reinterpret_cast<i32x4_t*>(Xs(buf) + (u >> 3) * PITCH + 8 * (u & 7)) = st.x[i];
    }
#pragma unroll
    for (int i = 0; i < WL; ++i) {
      const int u = tid + NT * i;
      *reinterpret_cast<i32x4_t*>(Ws(buf) + (u >> 3) * PITCH + 8 * (u & 7)) = st.w[i];
    }
  };

  // lane state: token tile m is token t0 + 32 m + lr
  ScoreRun run[MT];
  int tgt[MT];
  sw16_f32x16 acc[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    run[m] = score_empty();
    tgt[m] = t0 + 32 * m + lr < T ? a.target[t0 + 32 * m + lr] : -1;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
  }

  // a finished group: this lane's 16 logits per token tile into the running state (ids ascend with r,
  // and from group to group: a strict > keeps the lowest id), then clear the accumulators
  auto fold = [&](int grp) {
    const int n0 = grp * BNT + 32 * wave + 4 * lh;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      float gm = -__builtin_inff();
      int gi = 0;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = n0 + (r & 3) + 8 * (r >> 2);
        const float v = acc[m][r];
        if (n < V) {  // rows past the vocabulary never enter the maximum
          if (v > gm) {
            gm = v;
            gi = n;
          }
          if (n == tgt[m]) run[m].tl = v;
        }
      }
      if (gm > -__builtin_inff()) {
        const float M = fmaxf(run[m].m, gm);
        float s = run[m].s * expf(run[m].m - M);  // (exp(-inf) = 0: nothing seen so far)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (n0 + (r & 3) + 8 * (r >> 2) < V) s += expf(acc[m][r] - M);
        run[m].s = s;
        run[m].m = M;
        if (gm > run[m].bv) {
          run[m].bv = gm;
          run[m].bi = gi;
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
    }
  };

  // one step: `cur` held step s, already in LDS - refill it with step s + 3; run step s's MFMAs from
  // its LDS buffer; move `nxt` (step s + 1) into the other buffer, last read at step s - 1 behind that
  // step's barrier; at a group's last K step fold it (behind the barrier: the other waves go on)
  int cg = g0, ck = 0;
  auto step = [&](Stage& cur, const Stage& nxt, int s) {
    load_step(cur);
    if (s >= total) return;
    const int buf = s & 1;
#pragma unroll
    for (int kk = 0; kk < BK; kk += 16) {
      const i32x4_t wv = *reinterpret_cast<const i32x4_t*>(Ws(buf) + (32 * wave + lr) * PITCH + kk + 8 * lh);
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const i32x4_t xv = *reinterpret_cast<const i32x4_t*>(Xs(buf) + (32 * m + lr) * PITCH + kk + 8 * lh);
        if constexpr (F16)
          acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(sw16_f16x8, wv),
                                                          __builtin_bit_cast(sw16_f16x8, xv), acc[m], 0, 0, 0);
        else
          acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(sw16_bf16x8, wv),
                                                           __builtin_bit_cast(sw16_bf16x8, xv), acc[m], 0, 0, 0);
      }
    }
    if (s + 1 < total) store_step(nxt, buf ^ 1);
    __syncthreads();
    if (++ck == nk) {
      ck = 0;
      fold(cg++);
    }
  };

  Stage s0, s1, s2;
  load_step(s0);
  load_step(s1);
  load_step(s2);
  store_step(s0, 0);
  __syncthreads();
  for (int s = 0; s < total; s += 3) {
    step(s0, s1, s);
    step(s1, s2, s + 1);
    step(s2, s0, s + 2);
  }

  // ---- end of the range: lanes l and l ^ 32 hold the two halves of a token's rows; then the waves
  // (the last step's barrier closed every tile read: the buffers are free)
  ScoreRun* red = reinterpret_cast<ScoreRun*>(lds);
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    ScoreRun r = run[m];
    score_merge(r, score_shfl_xor(r, 32));
    if (lh == 0) red[wave * TM + 32 * m + lr] = r;
  }
  __syncthreads();
  if (tid < TM && t0 + tid < T) {
    ScoreRun r = red[tid];
#pragma unroll
    for (int w = 1; w < 4; ++w) score_merge(r, red[w * TM + tid]);  // a fixed order
    float* p = a.part + ((size_t)blockIdx.x * T + t0 + tid) * kScorePartWords;
    p[0] = r.m;
    p[1] = r.s;
    p[2] = r.tl;
    p[3] = r.bv;
    p[4] = __int_as_float(r.bi);
  }
}

// block shape and ranges as score_plan's (score.hip), over 128-row groups: TM = 64 up to 64 rows, else
// 128; ranges sized for about two resident rounds of blocks over the CUs
static void score_w16_plan(int T, int V, int pin, int& tm, int& ngroups, int& gpr, int& nranges) {
  tm = T > 64 ? 128 : 64;
  ngroups = (V + SW16_GROUP - 1) / SW16_GROUP;
  const int gy = (T + tm - 1) / tm;
  const int want = std::max(1, std::min(ngroups, 2 * bmm_cus() / gy));
  gpr = pin > 0 ? std::min(pin, ngroups) : (ngroups + want - 1) / want;
  nranges = (ngroups + gpr - 1) / gpr;
}

size_t score_head_w16_workspace_words(int T, int V, int gpr) {
  if (T < 1 || V < 1) throw std::runtime_error("score_head_w16: T and V must be positive");
  int tm, ngroups, g, nranges;
  score_w16_plan(T, V, gpr, tm, ngroups, g, nranges);
  return (size_t)nranges * (size_t)T * kScorePartWords;
}

template <bool F16>
static void launch_score_head_w16(const ScoreHeadArgs& a, int tm, int ngroups, int gpr, int nranges, hipStream_t s) {
  const dim3 grid(nranges, (a.T + tm - 1) / tm);
  if (tm == 128) hipLaunchKernelGGL((score_head_w16_kernel<F16, 128>), grid, dim3(256), 0, s, a, gpr, ngroups);
  else hipLaunchKernelGGL((score_head_w16_kernel<F16, 64>), grid, dim3(256), 0, s, a, gpr, ngroups);
  score_finish(a, nranges, s);
}

void score_head_w16(const ScoreHeadArgs& a, hipStream_t s) {
  if (a.w.type != T_BF16 && a.w.type != T_F16) throw std::runtime_error("score_head_w16: a BF16 or F16 head only");
  if (a.T < 1 || a.V < 1 || a.w.rows != a.V) throw std::runtime_error("score_head_w16: T >= 1 and rows = V >= 1");
  if (a.V >= (1 << 24)) throw std::runtime_error("score_head_w16: vocabulary ids must stay below 2^24");
  if (!a.w.base || !a.x || !a.target || !a.h_target || !a.part || !a.rec) throw std::runtime_error("score_head_w16: null buffer");
  if (a.w.K < SW16_BK || a.w.K % SW16_BK) throw std::runtime_error("score_head_w16: K must be a multiple of 64");
  if (reinterpret_cast<uintptr_t>(a.w.base) % 16 || reinterpret_cast<uintptr_t>(a.x) % 16 ||
      reinterpret_cast<uintptr_t>(a.rec) % 16 || reinterpret_cast<uintptr_t>(a.part) % 4 ||
      reinterpret_cast<uintptr_t>(a.target) % 4)
    throw std::runtime_error("score_head_w16: the head, X and the records must be 16-byte aligned");
  if (a.gpr < 0) throw std::runtime_error("score_head_w16: groups per range");
  int tm, ngroups, gpr, nranges;
  score_w16_plan(a.T, a.V, a.gpr, tm, ngroups, gpr, nranges);
  if ((size_t)nranges * (size_t)a.T * kScorePartWords > a.part_words)
    throw std::runtime_error("score_head_w16: the partial workspace is too small (score_head_w16_workspace_words)");
  for (int t = 0; t < a.T; ++t)
    if (a.h_target[t] < -1 || a.h_target[t] >= a.V)
      throw std::runtime_error("score_head_w16: target outside [0, V) and not -1");
  if (a.w.type == T_F16) launch_score_head_w16<true>(a, tm, ngroups, gpr, nranges, s);
  else launch_score_head_w16<false>(a, tm, ngroups, gpr, nranges, s);
}

}  // namespace lfk
