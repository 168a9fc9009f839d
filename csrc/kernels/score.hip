// The scoring head: prompt log-probabilities on the tile16 copy of the lm_head (kernels.h
// ScoreHeadArgs). A sibling of bmm.hip's gemm_t16_kernel over the same device pieces (t16_dev.h).
#include <algorithm>
#include <stdexcept>

#include "score_dev.h"
#include "t16_dev.h"

namespace lfk {

// ---------------------------------------------------------------- scoring head
// Prompt log-probabilities without the [T][V] logits (4096 rows x 128256 fp32 = 2.1 GB written and
// read back for three numbers per row). gemm_t16's main loop as it stands - X slice double
// buffered in LDS with the row swizzle, ping-pong raw weight tiles, A fragments that serve TM / 16
// token groups - but a block owns TM tokens x a contiguous RANGE of whole 256-row vocabulary groups
// (8 waves x 2 tiles) and loops over the groups of its range. After each group the accumulators
// hold (vocab row 16 tile + 4 kq + e, token t0 + 16 g + r16) and are reduced per token: in lane
// over e and the wave's two tiles, across kq by two cross-lane steps, across the waves through LDS
// (the X buffers are free then); thread t < TM carries token t's running (max, sum exp(l - max),
// target logit, best logit, best id) in registers over the range and stores ONE partial at
// part[range][t]. A finish launch (one wave per token) merges the ranges in a fixed order. Every
// merge is (max, rescaled sum): no logit is ever exponentiated without its maximum subtracted
// (ScoreRun, score_dev.h).
template <int QT, int TM>
__global__ __launch_bounds__(512) void score_head_kernel(ScoreHeadArgs a, int gpr, int ngroups) {
  constexpr int NWV = 8, NG = TM / 16, NT = NWV * 64;
  constexpr int XL = TM * 16 / NT;  // 16-B X pieces per thread per half step
  constexpr int SB = t16_step_bytes(QT);
  static_assert(XL == 2 || XL == 4, "X pieces per thread");
  __shared__ __attribute__((aligned(16))) __half xs[2][TM * kT16Pitch];
  __shared__ int tgt_s[TM];
  static_assert(sizeof(ScoreRun) * NWV * TM <= sizeof(xs), "the waves' reduction fits the X buffers");
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, kq = lane >> 4;
  const int K = a.w.K, steps = K >> 8, nh = 2 * steps;
  const int ntiles = a.w.rows >> 4;
  const int t0 = blockIdx.y * TM;
  const int g0 = blockIdx.x * gpr, g1 = min(ngroups, g0 + gpr);
  const size_t tstride = (size_t)steps * SB;
  if (tid < TM) tgt_s[tid] = t0 + tid < a.T ? a.target[t0 + tid] : -1;  // (read after the loop's barriers)
  // X as in gemm_t16_kernel: rows past T load row T - 1 (finite values, never stored)
  uint4 x0, x1, x2, x3;
  const auto rsx = __builtin_amdgcn_make_buffer_rsrc(const_cast<__half*>(a.x), 0, 0x7FFFFFFF, 0x00020000);
  int xvo[XL];
#pragma unroll
  for (int j = 0; j < XL; ++j) xvo[j] = (min(t0 + ((tid + NT * j) >> 4), a.T - 1) * K + 8 * (tid & 15)) * 2;
  auto xld = [&](int j, int k0) __attribute__((always_inline)) {
    return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rsx, xvo[j], k0 * 2, 0));
  };
  auto load_x = [&](int i) __attribute__((always_inline)) {
    const int k0 = 128 * i;
    x0 = xld(0, k0);
    x1 = xld(1, k0);
    if constexpr (XL > 2) x2 = xld(XL > 2 ? 2 : 0, k0);
    if constexpr (XL > 3) x3 = xld(XL > 3 ? 3 : 0, k0);
  };
  auto store_x = [&](int buf) __attribute__((always_inline)) {
    __half* d = &xs[buf][(tid >> 4) * kT16Pitch + 8 * ((tid & 15) ^ ((tid >> 4) & 15))];
    constexpr int J = (NT / 16) * kT16Pitch;
    *reinterpret_cast<uint4*>(d) = x0;
    *reinterpret_cast<uint4*>(d + J) = x1;
    if constexpr (XL > 2) *reinterpret_cast<uint4*>(d + 2 * J) = x2;
    if constexpr (XL > 3) *reinterpret_cast<uint4*>(d + 3 * J) = x3;
  };
  ScoreRun run = score_empty();  // thread tid < TM: token t0 + tid over this block's range
  ScoreRun* red = reinterpret_cast<ScoreRun*>(&xs[0][0]);
  for (int grp = g0; grp < g1; ++grp) {
    const int tile0 = grp * 2 * NWV + 2 * wave;  // this wave's tiles: tile0, tile0 + 1 (past the end: the last one, masked)
    const uint8_t* wt0 = a.w.base + (size_t)min(tile0, ntiles - 1) * tstride;
    const uint8_t* wt1 = a.w.base + (size_t)min(tile0 + 1, ntiles - 1) * tstride;
    const auto rw0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(wt0), 0, 0x7FFFFFFF, 0x00020000);
    const auto rw1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(wt1), 0, 0x7FFFFFFF, 0x00020000);
    f4_t acc[2][NG];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int g = 0; g < NG; ++g) acc[j][g] = f4_t{0.f, 0.f, 0.f, 0.f};
    auto load_w = [&](int i, BRawT<QT>& w0, BRawT<QT>& w1) __attribute__((always_inline)) {
      tload_rs<QT, false>(w0, rw0, (i >> 1) * SB, i & 1, lane, r16, kq);
      tload_rs<QT, false>(w1, rw1, (i >> 1) * SB, i & 1, lane, r16, kq);
    };
    auto half = [&](int i, const BRawT<QT>& w0, const BRawT<QT>& w1) __attribute__((always_inline)) {
      const int s = i >> 1, h = i & 1;
      const int c = 8 * s + 4 * h + kq;
      int off_lo, off_hi;
      chunk_runs<QT>(c, off_lo, off_hi);
      off_lo -= 256 * s + 128 * h;
      off_hi -= 256 * s + 128 * h;
      HFrag F0, F1;
      dequant_frags<QT>(w0, c, F0);
      dequant_frags<QT>(w1, c, F1);
      const __half* xb = &xs[i & 1][r16 * kT16Pitch];
#pragma unroll
      for (int g = 0; g < NG; ++g) {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const int u = (((m < 2 ? off_lo : off_hi) >> 3) + (m & 1)) ^ r16;  // swizzled 16-B unit
          const uint4 bv = *reinterpret_cast<const uint4*>(xb + g * 16 * kT16Pitch + 8 * u);
          const int dw = 2 * (m & 1), sh = (m >> 1) * 2;
          const uint4 a0 = make_uint4(F0.w[4 * dw + sh], F0.w[4 * dw + sh + 1], F0.w[4 * dw + 4 + sh], F0.w[4 * dw + 5 + sh]);
          const uint4 a1 = make_uint4(F1.w[4 * dw + sh], F1.w[4 * dw + sh + 1], F1.w[4 * dw + 4 + sh], F1.w[4 * dw + 5 + sh]);
          acc[0][g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8_t, a0), __builtin_bit_cast(h8_t, bv), acc[0][g], 0, 0, 0);
          acc[1][g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8_t, a1), __builtin_bit_cast(h8_t, bv), acc[1][g], 0, 0, 0);
        }
      }
    };
    BRawT<QT> wa0, wa1, wb0, wb1;
    load_x(0);
    load_w(0, wa0, wa1);
    store_x(0);
    lds_barrier();
    for (int i = 0; i < nh; i += 2) {  // (as gemm_t16_kernel: clamped repeats past the last half, no load under a branch)
      load_w(i + 1, wb0, wb1);
      load_x(i + 1);
      half(i, wa0, wa1);
      store_x((i + 1) & 1);
      lds_barrier();
      load_w(min(i + 2, nh - 1), wa0, wa1);
      load_x(min(i + 2, nh - 1));
      half(i + 1, wb0, wb1);
      store_x(i & 1);
      lds_barrier();
    }
    // ---- the group's 256 logits per token -> one ScoreRun per wave and token (ids ascend with j, e)
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const int tgt = tgt_s[16 * g + r16];
      ScoreRun r = score_empty();
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int n = 16 * (tile0 + j) + 4 * kq + e;
          const float v = acc[j][g][e];
          if (n < a.V) {  // tile padding (and the tiles past the end) never enter the maximum
            if (v > r.bv) {
              r.bv = v;
              r.bi = n;
            }
            if (n == tgt) r.tl = v;
          }
        }
      r.m = r.bv;
      if (r.m > -__builtin_inff()) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (16 * (tile0 + j) + 4 * kq + e < a.V) r.s += expf(acc[j][g][e] - r.m);
      }
      score_merge(r, score_shfl_xor(r, 16));
      score_merge(r, score_shfl_xor(r, 32));
      if (kq == 0) red[wave * TM + 16 * g + r16] = r;
    }
    lds_barrier();
    if (tid < TM) {
#pragma unroll
      for (int w = 0; w < NWV; ++w) score_merge(run, red[w * TM + tid]);  // wave order = ascending ids
    }
    lds_barrier();  // the next group's X goes where `red` was
  }
  if (tid < TM && t0 + tid < a.T) {
    float* p = a.part + ((size_t)blockIdx.x * a.T + t0 + tid) * kScorePartWords;
    p[0] = run.m;
    p[1] = run.s;
    p[2] = run.tl;
    p[3] = run.bv;
    p[4] = __int_as_float(run.bi);
  }
}

// stage 2: one wave per token. Lane l folds ranges l, l + 64, ... in ascending order, then the
// lanes meet in a fixed butterfly: the order is a function of the range count alone.
__global__ __launch_bounds__(256) void score_finish_kernel(ScoreHeadArgs a, int nranges) {
  const int lane = threadIdx.x & 63, t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= a.T) return;  // whole waves
  ScoreRun r = score_empty();
  for (int g = lane; g < nranges; g += 64) {
    const float* p = a.part + ((size_t)g * a.T + t) * kScorePartWords;
    score_merge(r, ScoreRun{p[0], p[1], p[2], p[3], __float_as_int(p[4])});
  }
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const ScoreRun o = score_shfl_xor(r, off);
    // both lanes of a pair must reach the same bits: merge (lower lane, upper lane) on either side
    ScoreRun lo = (lane & off) ? o : r;
    score_merge(lo, (lane & off) ? r : o);
    r = lo;
  }
  if (lane == 0) {
    const float lse = r.m + logf(r.s);
    const float lp = a.target[t] >= 0 ? r.tl - lse : __builtin_nanf("");
    *reinterpret_cast<float4*>(a.rec + (size_t)t * kScoreRecWords) =
        make_float4(lp, lse, __int_as_float(r.bi), r.bv - lse);
  }
}

void score_finish(const ScoreHeadArgs& a, int nranges, hipStream_t s) {
  hipLaunchKernelGGL(score_finish_kernel, dim3((a.T + 3) / 4), dim3(256), 0, s, a, nranges);
}

// block shape and ranges: TM = 64 up to 64 rows, else 128 (each token block streams the whole head
// once, so fewer blocks along T decode fewer weights); ranges sized for about two resident rounds
// of 512-thread blocks over the CUs
static void score_plan(int T, int V, int pin, int& tm, int& ngroups, int& gpr, int& nranges) {
  tm = T > 64 ? 128 : 64;
  ngroups = (V + 255) / 256;
  const int gy = (T + tm - 1) / tm;
  const int want = std::max(1, std::min(ngroups, 2 * bmm_cus() / gy));
  gpr = pin > 0 ? std::min(pin, ngroups) : (ngroups + want - 1) / want;
  nranges = (ngroups + gpr - 1) / gpr;
}

size_t score_head_workspace_words(int T, int V, int gpr) {
  if (T < 1 || V < 1) throw std::runtime_error("score_head: T and V must be positive");
  int tm, ngroups, g, nranges;
  score_plan(T, V, gpr, tm, ngroups, g, nranges);
  return (size_t)nranges * (size_t)T * kScorePartWords;
}

template <int QT>
static void launch_score_head(const ScoreHeadArgs& a, int tm, int ngroups, int gpr, int nranges, hipStream_t s) {
  const dim3 grid(nranges, (a.T + tm - 1) / tm);
  if (tm == 128) hipLaunchKernelGGL((score_head_kernel<QT, 128>), grid, dim3(512), 0, s, a, gpr, ngroups);
  else hipLaunchKernelGGL((score_head_kernel<QT, 64>), grid, dim3(512), 0, s, a, gpr, ngroups);
  score_finish(a, nranges, s);
}

void score_head(const ScoreHeadArgs& a, hipStream_t s) {
  if (a.T <= 0) return;
  if (!a.w.base || !a.x || !a.target || !a.h_target || !a.part || !a.rec) throw std::runtime_error("score_head: null buffer");
  if (a.w.K % 256 || a.w.K < 256 || !bmm_supported(a.w.type, a.w.K))
    throw std::runtime_error("score_head: the head needs a tile16 form (K a multiple of 256)");
  if (a.w.rows % 16 || a.V < 1 || a.V > a.w.rows || a.w.rows - a.V >= 16)
    throw std::runtime_error("score_head: the copy's rows are V padded to a multiple of 16");
  if ((long long)a.T * a.w.K * 2 >= (1LL << 31)) throw std::runtime_error("score_head: X exceeds the 2 GB buffer offsets");
  if (reinterpret_cast<uintptr_t>(a.x) % 16 || reinterpret_cast<uintptr_t>(a.rec) % 16 ||
      reinterpret_cast<uintptr_t>(a.part) % 4 || reinterpret_cast<uintptr_t>(a.target) % 4)
    throw std::runtime_error("score_head: X and the records must be 16-byte aligned");
  if (a.gpr < 0) throw std::runtime_error("score_head: groups per range");
  int tm, ngroups, gpr, nranges;
  score_plan(a.T, a.V, a.gpr, tm, ngroups, gpr, nranges);
  if ((size_t)nranges * (size_t)a.T * kScorePartWords > a.part_words)
    throw std::runtime_error("score_head: the partial workspace is too small (score_head_workspace_words)");
  for (int t = 0; t < a.T; ++t)
    if (a.h_target[t] < -1 || a.h_target[t] >= a.V) throw std::runtime_error("score_head: target outside [0, V) and not -1");
  LFK_DISPATCH(LFK_TYPES_T16, t16_kernel_type(a.w.type), throw std::runtime_error("score_head: unsupported weight type"),
               launch_score_head<QT>(a, tm, ngroups, gpr, nranges, s));
}

}  // namespace lfk
