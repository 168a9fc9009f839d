// Wide MoE (17 .. 256 experts, top-k up to 16: Qwen3-MoE's 8 of 128): the router, the per-expert row
// lists with their work list, and the grouped expert GEMM that runs every routed expert of one
// projection in ONE launch. moe.hip's kernels are shaped for "few experts" - an accumulator or a
// lane per expert, one block, a GEMM pair per expert - and stay as they are for E <= 16.
//
//   moe_router_wide       x rows (f32) -> RMSNorm * w_norm -> f32 router -> softmax, top-k, renormalise.
//                         The experts of a row are split over blocks (8 per block, 2 per wave): no
//                         single CU streams the 1 MB router. The last-arriving block of a row - an
//                         integer atomic on a per-row counter that it re-arms - finishes in one wave.
//   moe_route_group_wide  per-expert row lists in ascending token order from logits (or from the
//                         router's picks), over blocks of 16 tokens: per-block histograms, a scan over
//                         blocks and experts by the last-arriving block, then a fill launch. Also the
//                         work list: items (expert, first row, rows <= kMoeItemRows), none for an
//                         expert without rows.
//   moe_gemm_grouped      grid = (128 weight rows) x (item bound): a block reads its item, addresses its
//                         expert's tile16 copy and multiplies the item's gathered rows on
//                         v_mfma_f32_16x16x32_f16 (t16_dev.h's dequantisation). SwiGLU or plain store;
//                         the down form runs its whole K, so nothing is zeroed and nothing is added
//                         atomically: two runs are bit-equal.
#include <algorithm>
#include <stdexcept>

#include "moe_route_dev.h"
#include "t16_dev.h"

namespace lfk {

// every byte of an inter-block hand-off goes through agent-scope accesses (as the attention merge)
__device__ __forceinline__ void st_agent(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_agent(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float ld_agent(const float* p) {
  return __hip_atomic_load(const_cast<float*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int ld_agent(const int* p) {
  return __hip_atomic_load(const_cast<int*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// this block's stores are out, then ONE add: true in every thread of the last block to arrive
__device__ __forceinline__ bool last_arriver(int* counter, int n_blocks, int* s_flag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const int prev = __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *s_flag = prev == n_blocks - 1;
    if (prev == n_blocks - 1) st_agent(counter, 0);  // re-armed for the next launch
  }
  __syncthreads();
  return *s_flag != 0;
}

static constexpr int kWideMaxE = 256, kWideMaxK = 16, kWideVals = kWideMaxE / 64;

// One wave: v[j] = value of expert lane + 64 j (-inf past E) -> softmax, k rounds of wave arg-max
// (lowest id on a tie), the picks renormalised over their sum. Lane j < k returns pick j.
__device__ __forceinline__ void wide_topk(float (&v)[kWideVals], int E, int k, int lane, int& my_id, float& my_w) {
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < kWideVals; ++j) m = fmaxf(m, v[j]);
  m = wave_max(m);
  float p[kWideVals], s = 0.f;
#pragma unroll
  for (int j = 0; j < kWideVals; ++j) {
    p[j] = lane + 64 * j < E ? __expf(v[j] - m) : -1.f;
    s += fmaxf(p[j], 0.f);
  }
  s = wave_sum(s);
#pragma unroll
  for (int j = 0; j < kWideVals; ++j) p[j] = p[j] >= 0.f ? p[j] / s : -1.f;
  float sel_sum = 0.f;
  my_id = 0;
  my_w = 0.f;
  for (int r = 0; r < k; ++r) {
    float best = p[0];
    int bi = lane;
#pragma unroll
    for (int j = 1; j < kWideVals; ++j)
      if (p[j] > best) { best = p[j]; bi = lane + 64 * j; }  // (equal: the lower id stays)
    for (int o = 32; o > 0; o >>= 1) {
      const float ob = __shfl_xor(best, o);
      const int oi = __shfl_xor(bi, o);
      if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (lane == r) { my_id = bi; my_w = best; }
    sel_sum += best;
#pragma unroll
    for (int j = 0; j < kWideVals; ++j)
      if (bi == lane + 64 * j) p[j] = -1.f;
  }
  my_w /= sel_sum;
}

// ------------------------------------------------------------------ router
static constexpr int kRouterEpb = 8;  // experts per block: 4 waves x 2 (E = 128: 16 blocks per row)

// grid (ceil(E / 8), rows), 256 threads, d floats of LDS. raw [rows][E] and cnt [rows] are workspace
// (cnt zero before the first launch). ids / wout [rows][k]; logits [rows][E] optional.
__global__ __launch_bounds__(256) void moe_router_wide_kernel(const float* __restrict__ x, int ldx,
                                                              const float* __restrict__ nw, float eps,
                                                              const float* __restrict__ W, int d, int E, int k,
                                                              float* raw, int* cnt, float* logits, int* ids,
                                                              float* wout) {
  extern __shared__ __attribute__((aligned(16))) float xn[];  // x * w_norm
  __shared__ float red[4];
  __shared__ int s_last;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int row = blockIdx.y;
  x += (size_t)row * ldx;
  // every block of the row stages the same n and sums the same squares in the same order
  float ss = 0.f;
  for (int i = tid * 4; i < d; i += 1024) {
    const float4 xv = *reinterpret_cast<const float4*>(x + i);
    const float4 wv = *reinterpret_cast<const float4*>(nw + i);
    ss += route_ss4(xv);
    *reinterpret_cast<float4*>(xn + i) = make_float4(xv.x * wv.x, xv.y * wv.y, xv.z * wv.z, xv.w * wv.w);
  }
  ss = wave_sum_fast(ss);
  if (lane == 0) red[wave] = ss;
  __syncthreads();
  // this wave's experts: whole rows of W over d, 1 KB per load instruction
  for (int e = blockIdx.x * kRouterEpb + wave; e < min(E, (int)(blockIdx.x + 1) * kRouterEpb); e += 4) {
    const float* wr = W + (size_t)e * d;
    float acc = 0.f;
#pragma unroll 4
    for (int i = lane * 4; i < d; i += 256) {
      const float4 r = *reinterpret_cast<const float4*>(wr + i);
      const float4 n = *reinterpret_cast<const float4*>(xn + i);
      acc += route_dot4(n, r);
    }
    acc = wave_sum_fast(acc);
    if (lane == 0) st_agent(raw + (size_t)row * E + e, acc);
  }
  if (!last_arriver(cnt + row, gridDim.x, &s_last) || wave != 0) return;
  const float sc = rsqrtf(((red[0] + red[1]) + (red[2] + red[3])) / (float)d + eps);
  float v[kWideVals];
#pragma unroll
  for (int j = 0; j < kWideVals; ++j) {
    const int e = lane + 64 * j;
    v[j] = e < E ? ld_agent(raw + (size_t)row * E + e) * sc : -INFINITY;
    if (logits && e < E) logits[(size_t)row * E + e] = v[j];
  }
  int my_id;
  float my_w;
  wide_topk(v, E, k, lane, my_id, my_w);
  if (lane < k) {
    ids[row * k + lane] = my_id;
    wout[row * k + lane] = my_w;
  }
}

// workspace: the per-row counters first, at a place that does not move with the row count - launches of
// different row counts share one workspace, and each must find its counters re-armed - then raw [rows][E]
static constexpr int kRouterMaxRows = 4096;
size_t moe_router_wide_workspace(int rows, int E) { return sizeof(int) * kRouterMaxRows + sizeof(float) * (size_t)rows * E; }

bool moe_router_wide_ok(int router_type, int E, int k, int d) {
  return router_type == T_F32 && E > 16 && E <= kWideMaxE && k >= 1 && k <= kWideMaxK && k <= E && d % 4 == 0 &&
         d <= 15 * 1024;
}

void moe_router_wide(const float* x, int ldx, int rows, const float* nw, float eps, const float* W, int d, int E, int k,
                     void* ws, float* logits, int* ids, float* w, hipStream_t s) {
  if (rows < 1) return;
  if (!moe_router_wide_ok(T_F32, E, k, d) || ldx % 4 || ldx < d || !ws || rows > kRouterMaxRows)
    throw std::runtime_error("moe_router_wide: 17 .. 256 experts, k <= 16, d a multiple of 4 up to 15360, <= 4096 rows");
  int* cnt = reinterpret_cast<int*>(ws);
  float* raw = reinterpret_cast<float*>(cnt + kRouterMaxRows);
  hipLaunchKernelGGL(moe_router_wide_kernel, dim3((E + kRouterEpb - 1) / kRouterEpb, rows), dim3(256),
                     sizeof(float) * d, s, x, ldx, nw, eps, W, d, E, k, raw, cnt, logits, ids, w);
}

// ------------------------------------------------------------------ row lists and the work list
static constexpr int kGroupTok = 16;  // tokens per block

int moe_group_wide_items(int T, int E, int k) { return std::min(E, T * k) + T * k / kMoeItemRows; }
size_t moe_group_wide_workspace(int T, int E) {
  return sizeof(int) * ((size_t)((T + kGroupTok - 1) / kGroupTok) * E + 4);  // the counter first (fixed place), then hist
}

// Phase 1, grid ceil(T / 16) x 256 threads: top-k per token (one wave per token; skipped when the
// picks come in), this block's histogram -> hist[blk][E]; the last block to arrive turns hist into
// each block's first position per expert, and writes cnt_off and the work list.
__global__ __launch_bounds__(256) void moe_group_wide_count_kernel(const float* __restrict__ logits, int T, int E, int k,
                                                                   int* sel, float* selw, int* hist, int* counter,
                                                                   int* cnt_off, int* items, int* n_items) {
  __shared__ int s_hist[kWideMaxE];
  __shared__ int s_last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t0 = blockIdx.x * kGroupTok, t1 = min(T, t0 + kGroupTok);
  s_hist[tid] = 0;
  if (logits) {
    for (int t = t0 + wave; t < t1; t += 4) {
      float v[kWideVals];
#pragma unroll
      for (int j = 0; j < kWideVals; ++j) v[j] = lane + 64 * j < E ? logits[(size_t)t * E + lane + 64 * j] : -INFINITY;
      int my_id;
      float my_w;
      wide_topk(v, E, k, lane, my_id, my_w);
      if (lane < k) {
        sel[t * k + lane] = my_id;
        selw[t * k + lane] = my_w;
      }
    }
  }
  __syncthreads();  // (the picks written above are read back by their own block: visible after the barrier)
  for (int i = t0 * k + tid; i < t1 * k; i += 256) atomicAdd(&s_hist[sel[i]], 1);  // integer counts: order-free
  __syncthreads();
  if (tid < E) st_agent(hist + (size_t)blockIdx.x * E + tid, s_hist[tid]);
  if (!last_arriver(counter, gridDim.x, &s_last)) return;
  // scan over blocks: hist[b][e] becomes the rows of expert e in blocks before b
  int total = 0;
  if (tid < E)
    for (int b = 0; b < (int)gridDim.x; ++b) {
      int* h = hist + (size_t)b * E + tid;
      const int c = ld_agent(h);
      *h = total;
      total += c;
    }
  s_hist[tid] = total;
  __syncthreads();
  if (wave != 0) return;
  // scan over experts, one wave, four consecutive experts per lane: offsets and first item index
  int c[4], off = 0, it = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    c[j] = s_hist[4 * lane + j];
    off += c[j];
    it += (c[j] + kMoeItemRows - 1) / kMoeItemRows;
  }
  int offs = off, its = it;  // inclusive scans over the lanes
  for (int o = 1; o < 64; o <<= 1) {
    const int a = __shfl_up(offs, o), b = __shfl_up(its, o);
    if (lane >= o) { offs += a; its += b; }
  }
  if (lane == 63) {
    *n_items = its;
    cnt_off[E] = offs;  // T k
  }
  off = offs - off;
  it = its - it;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int e = 4 * lane + j;
    if (e < E) cnt_off[e] = off;
    for (int r = 0; r < c[j]; r += kMoeItemRows, ++it) {
      items[3 * it] = e;
      items[3 * it + 1] = off + r;
      items[3 * it + 2] = min(kMoeItemRows, c[j] - r);
    }
    off += c[j];
  }
}

// Phase 2, same grid: thread e walks its block's picks in token order and places expert e's rows
__global__ __launch_bounds__(256) void moe_group_wide_fill_kernel(int T, int E, int k, const int* __restrict__ sel,
                                                                  const float* __restrict__ selw,
                                                                  const int* __restrict__ hist,
                                                                  const int* __restrict__ cnt_off, int* tok, float* gw,
                                                                  int* pos) {
  __shared__ int s_sel[kGroupTok * kWideMaxK];
  const int tid = threadIdx.x;
  const int i0 = blockIdx.x * kGroupTok * k, n = (min(T, (int)(blockIdx.x + 1) * kGroupTok)) * k - i0;
  if (tid < n) s_sel[tid] = sel[i0 + tid];
  __syncthreads();
  if (tid >= E) return;
  int p = cnt_off[tid] + hist[(size_t)blockIdx.x * E + tid];
  for (int i = 0; i < n; ++i)
    if (s_sel[i] == tid) {
      tok[p] = (i0 + i) / k;
      gw[p] = selw[i0 + i];
      pos[i0 + i] = p;
      ++p;
    }
}

void moe_route_group_wide(const float* logits, int T, int E, int k, int* sel, float* selw, int* cnt_off, int* tok,
                          float* gw, int* pos, int* items, int* n_items, void* ws, hipStream_t s) {
  if (T <= 0) return;
  if (E < 1 || E > kWideMaxE || k < 1 || k > kWideMaxK || k > E || !ws)
    throw std::runtime_error("moe_route_group_wide: n_expert <= 256, k <= 16");
  const int nb = (T + kGroupTok - 1) / kGroupTok;
  int* counter = reinterpret_cast<int*>(ws);
  int* hist = counter + 4;
  hipLaunchKernelGGL(moe_group_wide_count_kernel, dim3(nb), dim3(256), 0, s, logits, T, E, k, sel, selw, hist, counter,
                     cnt_off, items, n_items);
  hipLaunchKernelGGL(moe_group_wide_fill_kernel, dim3(nb), dim3(256), 0, s, T, E, k, sel, selw, hist, cnt_off, tok, gw,
                     pos);
}

// ------------------------------------------------------------------ grouped expert GEMM
// Block = 4 waves x 2 tiles (128 weight rows) x one item (<= 32 gathered rows = two MFMA column
// groups). Per 128-k half step the item's rows are staged in LDS (double buffered, swizzled as
// gemm_t16's), each wave's two tiles' raw weights run one half ahead (ping-pong) and are dequantised
// once per half into A fragments that serve both column groups.
template <int QT, int EPI, bool NTQ>
__global__ __launch_bounds__(256) void moe_gemm_grouped_kernel(MoeGroupedArgs a) {
  constexpr int TM = kMoeItemRows, NG = TM / 16, NT = 256, XL = TM * 16 / NT;
  constexpr int SB = t16_step_bytes(QT);
  static_assert(XL == 2, "two 16-B X pieces per thread per half step");
  if ((int)blockIdx.y >= *a.n_items) return;  // whole block, before any load of weights or rows
  __shared__ __attribute__((aligned(16))) __half xs[2][TM * kT16Pitch];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, kq = lane >> 4;
  const int e = __builtin_amdgcn_readfirstlane(a.items[3 * blockIdx.y]);
  const int r0 = __builtin_amdgcn_readfirstlane(a.items[3 * blockIdx.y + 1]);
  const int n = __builtin_amdgcn_readfirstlane(a.items[3 * blockIdx.y + 2]);
  const int K = a.K, steps = K >> 8, nh = 2 * steps;
  const int ntiles = a.rows >> 4;
  const int tile0 = blockIdx.x * 8 + 2 * wave;
  auto tile_base = [&](int t) __attribute__((always_inline)) {
    return a.w + (size_t)e * a.expert_bytes + (size_t)min(t, ntiles - 1) * a.tile_stride + (size_t)e * a.expert_step0 * SB;
  };
  const auto rw0 = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(tile_base(tile0)), 0, 0x7FFFFFFF, 0x00020000);
  const auto rw1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(tile_base(tile0 + 1)), 0, 0x7FFFFFFF, 0x00020000);
  // rows past the item's last load its last row: finite values whose outputs are never stored
  const __half* xi = a.x + (size_t)r0 * K;
  const auto rsx = __builtin_amdgcn_make_buffer_rsrc(const_cast<__half*>(xi), 0, 0x7FFFFFFF, 0x00020000);
  int xvo[XL];  // (an item's rows: 32 x K x 2 bytes)
#pragma unroll
  for (int j = 0; j < XL; ++j) xvo[j] = (min((tid + NT * j) >> 4, n - 1) * K + 8 * (tid & 15)) * 2;
  uint4 x0, x1;
  auto load_x = [&](int i) __attribute__((always_inline)) {
    const int k0 = (i >> 1) * 256 + 128 * (i & 1);
    x0 = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rsx, xvo[0], k0 * 2, 0));
    x1 = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rsx, xvo[1], k0 * 2, 0));
  };
  auto store_x = [&](int buf) __attribute__((always_inline)) {
    __half* d = &xs[buf][(tid >> 4) * kT16Pitch + 8 * ((tid & 15) ^ ((tid >> 4) & 15))];
    *reinterpret_cast<uint4*>(d) = x0;
    *reinterpret_cast<uint4*>(d + (NT / 16) * kT16Pitch) = x1;
  };
  auto load_w = [&](int i, BRawT<QT>& w0, BRawT<QT>& w1) __attribute__((always_inline)) {
    tload_rs<QT, NTQ>(w0, rw0, (i >> 1) * SB, i & 1, lane, r16, kq);
    tload_rs<QT, NTQ>(w1, rw1, (i >> 1) * SB, i & 1, lane, r16, kq);
  };
  f4_t acc[2][NG];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int g = 0; g < NG; ++g) acc[j][g] = f4_t{0.f, 0.f, 0.f, 0.f};
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
  // (as gemm_t16: the loads past the last half are clamped repeats, no load under a branch)
  for (int i = 0; i < nh; i += 2) {
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
  // acc[j][g][c] = (weight row 16 (tile0 + j) + 4 kq + c, item row 16 g + r16)
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int tile = tile0 + j;
    if (tile >= ntiles) continue;  // wave-uniform
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const int t = 16 * g + r16;
      const f4_t v = acc[j][g];
      if constexpr (EPI == GEMM_SWIGLU) {  // the tile = 8 gate + 8 up rows of features 8 tile ..
        f4_t u;
#pragma unroll
        for (int c = 0; c < 4; ++c) u[c] = __shfl_xor(v[c], 32);
        const int f = 8 * tile + 4 * kq;
        if (kq < 2 && t < n) {
          float hv[4];
#pragma unroll
          for (int c = 0; c < 4; ++c) hv[c] = v[c] / (1.f + __expf(-v[c])) * u[c];
          const __half2 p0 = __floats2half2_rn(hv[0], hv[2]), p1 = __floats2half2_rn(hv[1], hv[3]);
          *reinterpret_cast<uint2*>(a.out_h + (size_t)(r0 + t) * a.ld + f) =
              make_uint2(__builtin_bit_cast(unsigned, p0), __builtin_bit_cast(unsigned, p1));
        }
      } else if (t < n) {
        *reinterpret_cast<float4*>(a.out + (size_t)(r0 + t) * a.ld + 16 * tile + 4 * kq) = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
  }
}

template <int QT>
static void launch_moe_grouped(const MoeGroupedArgs& a, hipStream_t s) {
  const dim3 grid((a.rows / 16 + 7) / 8, a.max_items);
  // max_items = min(E, T k) + T k / 32 <= E means T k <= ~E: a row or two per routed expert (decode), every
  // weight read once - non-temporal. Past it (a 512-token chunk at 8 of 128: 256 items) several items
  // and row groups re-read an expert's tiles through the cache. (The switch point is reasoned, not measured.)
  const bool nt = a.max_items <= a.n_expert;
  if (a.swiglu) {
    if (nt) hipLaunchKernelGGL((moe_gemm_grouped_kernel<QT, GEMM_SWIGLU, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((moe_gemm_grouped_kernel<QT, GEMM_SWIGLU, false>), grid, dim3(256), 0, s, a);
  } else {
    if (nt) hipLaunchKernelGGL((moe_gemm_grouped_kernel<QT, GEMM_STORE, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((moe_gemm_grouped_kernel<QT, GEMM_STORE, false>), grid, dim3(256), 0, s, a);
  }
}

bool moe_gemm_grouped_ok(int type, int rows, int K) { return bmm_supported(type, K) && rows % 16 == 0 && rows >= 16; }

void moe_gemm_grouped(const MoeGroupedArgs& a, hipStream_t s) {
  if (a.max_items < 1) return;
  if (!moe_gemm_grouped_ok(a.type, a.rows, a.K) || !a.w || !a.x || !a.items || !a.n_items || a.n_expert < 1)
    throw std::runtime_error("moe_gemm_grouped: unsupported type / shape");
  if (reinterpret_cast<uintptr_t>(a.x) % 16 || a.ld % 4 || (a.swiglu ? !a.out_h || a.ld < a.rows / 2 : !a.out || a.ld < a.rows))
    throw std::runtime_error("moe_gemm_grouped: rows / output");
  if (a.max_items > 65535) throw std::runtime_error("moe_gemm_grouped: more than 65535 items");
  LFK_DISPATCH(LFK_TYPES_T16, t16_kernel_type(a.type), throw std::runtime_error("moe_gemm_grouped: unsupported weight type"),
               launch_moe_grouped<QT>(a, s));
}

// p[0, n) = 0 (n % 4 == 0, p 16-byte aligned): the batched step's grouped FFN has no down projection
// whose blocks could re-zero the split-K Q|K|V sums as a side job. A kernel and not hipMemsetAsync: the
// step is captured, and memset nodes have replayed unreliably in captured graphs on some ROCm runtimes,
// while a kernel node is what every other node of the step is (a precaution, taken for the new path only)
__global__ void zero_f32_kernel(float4* p, int n4) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n4) p[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}
void zero_f32(float* p, size_t n, hipStream_t s) {
  if (!n) return;
  if (n % 4 || reinterpret_cast<uintptr_t>(p) % 16 || n / 4 > 0x7FFFFFFF) throw std::runtime_error("zero_f32: alignment");
  hipLaunchKernelGGL(zero_f32_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, s,
                     reinterpret_cast<float4*>(p), (int)(n / 4));
}

MoeGroupedArgs moe_grouped_gate_up_args(const uint8_t* t_gu, int type, int F, int d, int n_expert, const __half* xg,
                                        __half* h, const int* items, const int* n_items, int max_items) {
  MoeGroupedArgs a;
  a.w = t_gu; a.type = type; a.rows = 2 * F; a.K = d; a.n_expert = n_expert;
  a.tile_stride = t16_bytes(type, 16, d);
  a.expert_bytes = t16_bytes(type, 2 * F, d);  // the experts' SwiGLU copies back to back
  a.x = xg; a.out_h = h; a.ld = F; a.swiglu = true;
  a.items = items; a.n_items = n_items; a.max_items = max_items;
  return a;
}

MoeGroupedArgs moe_grouped_down_args(const uint8_t* t_down, int type, int d, int F, int n_expert, const __half* h,
                                     float* y, const int* items, const int* n_items, int max_items) {
  MoeGroupedArgs a;
  a.w = t_down; a.type = type; a.rows = d; a.K = F; a.n_expert = n_expert;
  a.tile_stride = t16_bytes(type, 16, F) * n_expert;  // one tile over all experts' K
  a.expert_step0 = F / 256;
  a.x = h; a.out = y; a.ld = d;
  a.items = items; a.n_items = n_items; a.max_items = max_items;
  return a;
}

}  // namespace lfk
