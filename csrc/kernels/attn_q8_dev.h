// Device bodies of the Q8_0 KV cache kernels (attention_q8.hip; the layout is described there).
// The split-L decode keeps attn_dev.h's block shape, wave-local softmax and last-arriver merge; what
// differs is how a key / value row reaches the arithmetic: 16-byte int8 loads, converted in
// registers, the block scale applied once per partial dot (K) or once per loaded value (V).
#pragma once
#include <cfloat>

#include "attn_dev.h"

namespace lfk {

// the planes of one layer of one slot: int8 [n_kv_head][n_ctx][HD], then f16 [n_kv_head][n_ctx][HD / 32]
template <int HD>
__device__ __forceinline__ const __half* q8_scales(const char* cache, int n_kv_head, int n_ctx) {
  return reinterpret_cast<const __half*>(cache + (size_t)n_kv_head * n_ctx * HD);
}

// 4 int8 -> 2 f16 pairs, exactly: u = q + 128 (one xor for the four), 0x6400 | u is the f16
// 1024 + u, and a packed subtract of 1152 leaves q. lo = bytes 0, 1; hi = bytes 2, 3.
__device__ __forceinline__ void q8_cvt4(unsigned w, h2v& lo, h2v& hi) {
  const unsigned u = w ^ 0x80808080u;
  const unsigned p0 = (u & 0xFFu) | ((u & 0xFF00u) << 8) | 0x64006400u;
  const unsigned p1 = ((u >> 16) & 0xFFu) | ((u >> 8) & 0xFF0000u) | 0x64006400u;
  const h2v off = {(_Float16)1152.f, (_Float16)1152.f};
  lo = __builtin_bit_cast(h2v, p0) - off;
  hi = __builtin_bit_cast(h2v, p1) - off;
}

__device__ __forceinline__ v4u q8_ld_nt(const char* p) {
  return __builtin_nontemporal_load(reinterpret_cast<const v4u*>(p));
}

// One block = 64 keys of one kv head x all G query heads; 4 waves of 16 keys, lane = (key = lane / 4,
// sub = lane % 4) holding HD / 4 int8 dims of its key: one whole Q8_0 block at HD 128, half of one at
// HD 64 - either way ONE scale per lane, folded into the lane's partial dot before the quad sum. q and
// the dot stay f32: there is no activation rounding term (and no int8-q v_dot4 route, which adds one).
// P.V: the wave's 16 value rows sit in LDS as int8 beside their scales as f32 (0 for a key past the
// length: a stale row's scale may be NaN, its int8 values cannot); a lane owns HD / 64 adjacent dims
// of one block and dequantises each loaded value once for all G heads.
template <int HD, int G>
__device__ __forceinline__ void attn_decode_q8_body(AttnDecodeArgs a) {
  constexpr int DPL = HD / 4;    // dims (= bytes) per lane in QK
  constexpr int NLD = DPL / 16;  // 16-B loads per lane per K (or V) row
  constexpr int KPW = 16;        // keys per wave
  constexpr int NB = HD / 32;    // Q8_0 blocks per row
  const char* kc = reinterpret_cast<const char*>(a.k_cache);
  const char* vc = reinterpret_cast<const char*>(a.v_cache);
  if (a.batch > 0) {  // batched decode: this row's query, KV slot, position, workspaces and output
    const int b = blockIdx.z;
    const size_t so = (size_t)a.slots[b] * a.slot_stride * sizeof(__half);
    a.q += (size_t)b * a.q_stride;
    kc += so;
    vc += so;
    a.pos += b;
    a.part += (size_t)b * a.part_stride;
    a.counters += 64 * b;
    if (a.out) a.out += (size_t)b * a.out_stride;
    if (a.out_h) a.out_h += (size_t)b * a.out_h_stride;
  }
  const int kvh = blockIdx.x, split = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kw = lane >> 2, sub = lane & 3;
  const int start = split * CH;
  const int key = start + wave * KPW + kw;

  // q * scale in f32 (an f16 q missed the 5e-3 bound at logits near 90: 7.9e-3 measured); the slice of
  // each sub skewed by 4 floats, so that the four subs' 16-byte reads fall on different banks
  __shared__ __attribute__((aligned(16))) float qs[G][HD + 16];
  __shared__ __attribute__((aligned(16))) signed char vs[4][KPW][HD + 16];
  __shared__ float vd[4][KPW][NB];
  __shared__ __attribute__((aligned(16))) float ps[4][G][KPW];
  __shared__ float wm[4][G], wl[4][G];
  __shared__ __attribute__((aligned(16))) float wo[4][G][HD];
  __shared__ int last;

  // ---- 1. loads: q, then the K / V rows and their scales, clamped to the cache (speculative: they
  //      do not wait for the device-resident position)
  constexpr int QPT = (G * HD / 2 + 255) / 256;  // q pairs per thread
  float2 qv[QPT];
#pragma unroll
  for (int j = 0; j < QPT; ++j)
    qv[j] = reinterpret_cast<const float2*>(a.q + (size_t)kvh * G * HD)[min(tid + 256 * j, G * HD / 2 - 1)];
  const size_t krow = (size_t)kvh * a.n_ctx + min(key, a.n_ctx - 1);
  v4u kr[NLD], vr[NLD];
#pragma unroll
  for (int i = 0; i < NLD; ++i) kr[i] = q8_ld_nt(kc + krow * HD + sub * DPL + 16 * i);
  const __half kdh = q8_scales<HD>(kc, a.n_kv_head, a.n_ctx)[krow * NB + (sub * DPL) / 32];
#pragma unroll
  for (int i = 0; i < NLD; ++i) vr[i] = q8_ld_nt(vc + krow * HD + sub * DPL + 16 * i);
  const __half vdh = q8_scales<HD>(vc, a.n_kv_head, a.n_ctx)[krow * NB + min(sub, NB - 1)];
#pragma unroll
  for (int j = 0; j < QPT; ++j) {
    const int i = tid + 256 * j;
    const int d = 2 * (i % (HD / 2));
    if (i < G * HD / 2)
      *reinterpret_cast<float2*>(&qs[i / (HD / 2)][d + 4 * (d / DPL)]) = make_float2(qv[j].x * a.scale, qv[j].y * a.scale);
  }
  const int L = min(*a.pos + 1, a.n_ctx);
  if (start >= L) return;
  const int ns = (L + CH - 1) / CH;
  __syncthreads();  // qs

  // ---- 2a. scores: the lane's int8 slice converted once to f32 for all G heads, the partial dot
  //      times the slice's one scale
  const bool valid = key < L;
  float kf[DPL];
#pragma unroll
  for (int i = 0; i < NLD; ++i)
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int u = (int)kr[i][w];
      kf[16 * i + 4 * w] = (float)((u << 24) >> 24);
      kf[16 * i + 4 * w + 1] = (float)((u << 16) >> 24);
      kf[16 * i + 4 * w + 2] = (float)((u << 8) >> 24);
      kf[16 * i + 4 * w + 3] = (float)(u >> 24);
    }
  const float kd = __half2float(kdh);
  float sc[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const float4* q4 = reinterpret_cast<const float4*>(&qs[g][sub * (DPL + 4)]);
    float p0 = 0.f, p1 = 0.f;
#pragma unroll
    for (int i = 0; i < DPL / 4; ++i) {
      const float4 qq = q4[i];
      p0 += qq.x * kf[4 * i];
      p1 += qq.y * kf[4 * i + 1];
      p0 += qq.z * kf[4 * i + 2];
      p1 += qq.w * kf[4 * i + 3];
    }
    sc[g] = quad_sum((p0 + p1) * kd);
  }
  // ---- 2b. wave-local softmax over the wave's 16 keys
  float mw[G], lw[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const float s = valid ? sc[g] : -FLT_MAX;
    mw[g] = rows_max(rowq_max(s));
    const float e = valid ? __expf(s - mw[g]) : 0.f;
    sc[g] = e;
    lw[g] = rows_sum(rowq_sum(e));
  }
  if (sub == 0) {
#pragma unroll
    for (int g = 0; g < G; ++g) ps[wave][g][kw] = sc[g];
  }
  // this wave's V rows (the wave's own keys: a wave barrier, no block barrier)
#pragma unroll
  for (int i = 0; i < NLD; ++i) *reinterpret_cast<v4u*>(&vs[wave][kw][sub * DPL + 16 * i]) = vr[i];
  if (sub < NB) vd[wave][kw][sub] = valid ? __half2float(vdh) : 0.f;
  // ---- 2c. P.V over this wave's keys (LDS written by this wave only)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  constexpr int DV = HD / 64;  // dims per lane in PV (1 or 2), all of block (DV * lane) / 32
  float o[G][DV];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int j = 0; j < DV; ++j) o[g][j] = 0.f;
#pragma unroll
  for (int k4 = 0; k4 < KPW; k4 += 4) {
    float4 pg[G];
#pragma unroll
    for (int g = 0; g < G; ++g) pg[g] = *reinterpret_cast<const float4*>(&ps[wave][g][k4]);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int k = k4 + kk;
      const float d = vd[wave][k][(DV * lane) / 32];
      float v[DV];
      if constexpr (DV == 2) {
        const unsigned short u = *reinterpret_cast<const unsigned short*>(&vs[wave][k][2 * lane]);
        v[0] = (float)(signed char)(u & 0xFF) * d;
        v[1] = (float)(signed char)(u >> 8) * d;
      } else {
        v[0] = (float)vs[wave][k][lane] * d;
      }
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const float p = kk == 0 ? pg[g].x : kk == 1 ? pg[g].y : kk == 2 ? pg[g].z : pg[g].w;
#pragma unroll
        for (int j = 0; j < DV; ++j) o[g][j] += p * v[j];
      }
    }
  }
#pragma unroll
  for (int g = 0; g < G; ++g) {
#pragma unroll
    for (int j = 0; j < DV; ++j) wo[wave][g][DV * lane + j] = o[g][j];
    if (lane == 0) {
      wm[wave][g] = mw[g];
      wl[wave][g] = lw[g];
    }
  }
  __syncthreads();
  // ---- 3. block partial: a pair of adjacent dims per thread (8-byte sc1 stores; (M, l) one pair too)
  for (int e2 = tid; e2 < G * HD / 2; e2 += 256) {
    const int g = (2 * e2) / HD, d = (2 * e2) % HD;
    const float M = fmaxf(fmaxf(wm[0][g], wm[1][g]), fmaxf(wm[2][g], wm[3][g]));
    float l = 0.f, acc0 = 0.f, acc1 = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float f = wm[w][g] == -FLT_MAX ? 0.f : __expf(wm[w][g] - M);
      l += f * wl[w][g];
      acc0 += f * wo[w][g][d];
      acc1 += f * wo[w][g][d + 1];
    }
    if (ns == 1) {
      const int o1 = (kvh * G + g) * HD + d;
      if (a.out) {
        a.out[o1] = acc0 / l;
        a.out[o1 + 1] = acc1 / l;
      }
      if (a.out_h) {
        a.out_h[swz4(o1)] = __float2half(acc0 / l);
        a.out_h[swz4(o1 + 1)] = __float2half(acc1 / l);
      }
    } else {
      float* dst = a.part + ((size_t)split * a.n_head + kvh * G + g) * (HD + 2);
      st2_sc1(dst + d, acc0, acc1);
      if (d == 0) st2_sc1(dst + HD, M, l);
    }
  }
  if (ns == 1) return;

  // ---- 4. hand-off: the last arriving block of this kv head merges all splits (attn_dev.h, step 4)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    const int prev = __hip_atomic_fetch_add(a.counters + kvh, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = (prev == ns - 1);
    if (last) __hip_atomic_store(a.counters + kvh, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (!last) return;
  constexpr int NSB = 16;
  for (int e2 = tid; e2 < G * HD / 2; e2 += 256) {  // a pair of adjacent dims of one head per thread
    const int h = kvh * G + (2 * e2) / HD, d0 = (2 * e2) % HD;
    float M = -FLT_MAX, n0 = 0.f, n1 = 0.f, den = 0.f;
    for (int s0 = 0; s0 < ns; s0 += NSB) {
      float2 st[NSB], pv[NSB];
#pragma unroll
      for (int i = 0; i < NSB; ++i) {  // one batch of independent sc1 loads per 16 splits
        const float* p = a.part + ((size_t)min(s0 + i, ns - 1) * a.n_head + h) * (HD + 2);
        st[i] = ld2_sc1(p + HD);
        pv[i] = ld2_sc1(p + d0);
      }
      float mb = M;
#pragma unroll
      for (int i = 0; i < NSB; ++i) mb = (s0 + i < ns) ? fmaxf(mb, st[i].x) : mb;
      const float r = __expf(M - mb);
      den *= r;
      n0 *= r;
      n1 *= r;
#pragma unroll
      for (int i = 0; i < NSB; ++i) {
        const float f = (s0 + i < ns) ? __expf(st[i].x - mb) : 0.f;
        den += f * st[i].y;
        n0 += f * pv[i].x;
        n1 += f * pv[i].y;
      }
      M = mb;
    }
    const int o1 = h * HD + d0;
    if (a.out) {
      a.out[o1] = n0 / den;
      a.out[o1 + 1] = n1 / den;
    }
    if (a.out_h) {
      a.out_h[swz4(o1)] = __float2half(n0 / den);
      a.out_h[swz4(o1 + 1)] = __float2half(n1 / den);
    }
  }
}

}  // namespace lfk
