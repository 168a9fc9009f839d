// Q8_0 KV cache (EngineOptions::kv_type "q8_0"; llama.cpp's type_k / type_v = 8): one writer and
// two readers.
//
// Cache layout, per layer and slot, K and V alike (planar, like the weight repack):
//   int8  [n_kv_head][n_ctx][head_dim]        the quantised values
//   f16   [n_kv_head][n_ctx][head_dim / 32]   one scale per 32-value block along head_dim
// the scale plane directly behind the int8 plane (n_kv_head n_ctx head_dim bytes in). A block is
// GGML's Q8_0: d = f16(amax / 127), q = round-to-nearest(x / d), an all-zero block d = 0, q = 0.
// 34 bytes per 32 values against 64: 0.53125 of the f16 cache. head_dim is 64 or 128, so an int8 row
// is one or two 64-byte segments and starts 64-byte aligned. Slot strides are counted in halves
// (2-byte units) like the f16 cache's, so that the engine's slot arithmetic is one and the same.
//
//   rope_kv_append_q8   raw Q|K|V sums -> (bias | head norm) -> RoPE -> q as f32, K / V quantised.
//                       One wave per head of one token, a lane per value (two at head_dim 128): a
//                       32-lane half-wave owns one block, its amax is five shuffle steps, the
//                       32 bytes of a block leave as one coalesced store. Nothing passes through LDS.
//   attn_decode_q8      split-L decode over the int8 rows (attn_q8_dev.h).
//   attn_prefill_q8     the MFMA flash kernel of attention.hip with another tile load: int8 chunks
//                       and their scales in flight in registers, converted to f16 on the way into
//                       the K / V tiles in LDS. The MFMA loop is the f16 kernel's.
#include <algorithm>
#include <cmath>
#include <stdexcept>

#include "attn_q8_dev.h"
#include "kernels.h"

namespace lfk {

// ---------------------------------------------------------------- append
template <int HD, bool NORM, bool BIAS>
__global__ __launch_bounds__(256) void rope_kv_append_q8_kernel(KvAppendQ8Args a) {
  constexpr int NV = HD / 64;  // values per lane: dims lane and lane + 64
  const int t = blockIdx.x, lane = threadIdx.x & 63;
  const int nhq = a.n_q / HD, nhk = a.n_kv / HD;
  const int h = blockIdx.y * 4 + (threadIdx.x >> 6);  // wave-uniform
  if (h >= nhq + 2 * nhk) return;
  const int pos = a.pos_arr ? min(max(a.pos_arr[t], 0), a.n_ctx - 1)
                            : a.pos_dev ? min(max(*a.pos_dev, 0), a.n_ctx - 1) : a.pos0 + t;
  const size_t col = (size_t)h * HD;
  const float* row = a.qkv + (size_t)t * (a.n_q + 2 * a.n_kv) + col;
  float x[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    x[j] = row[lane + 64 * j];
    if constexpr (BIAS) x[j] += a.bias[col + lane + 64 * j];
  }
  if (h < nhq + nhk) {  // q or k: (head norm,) then the rotation of adjacent pairs
    if constexpr (NORM) {
      float ss = 0.f;
#pragma unroll
      for (int j = 0; j < NV; ++j) ss += x[j] * x[j];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
      const float sc = rsqrtf(ss * (1.f / HD) + a.eps);
      const float* w = a.qk_norm + (h < nhq ? 0 : HD);
#pragma unroll
      for (int j = 0; j < NV; ++j) x[j] = x[j] * sc * w[lane + 64 * j];
    }
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const float other = __shfl_xor(x[j], 1);
      const float2 cs = a.rope[(size_t)pos * (HD / 2) + ((lane + 64 * j) >> 1)];
      x[j] = (lane & 1) ? other * cs.y + x[j] * cs.x : x[j] * cs.x - other * cs.y;
    }
  }
  if (h < nhq) {
#pragma unroll
    for (int j = 0; j < NV; ++j) a.q_out[(size_t)t * a.n_q + col + lane + 64 * j] = x[j];
    return;
  }
  const bool isk = h < nhq + nhk;
  const int kvh = isk ? h - nhq : h - nhq - nhk;
  char* cache = reinterpret_cast<char*>(isk ? a.k_cache : a.v_cache);
  if (a.slot_arr) cache += (size_t)a.slot_arr[t] * a.slot_stride * sizeof(__half);
  __half* scales = reinterpret_cast<__half*>(cache + (size_t)(a.n_kv / HD) * a.n_ctx * HD);
  const size_t r = (size_t)kvh * a.n_ctx + pos;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    float amax = fabsf(x[j]);
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));  // the half-wave's block
    const __half dh = __float2half(amax * (1.f / 127.f));
    const float d = __half2float(dh);
    const float q = fminf(fmaxf(rintf(d > 0.f ? x[j] / d : 0.f), -127.f), 127.f);
    cache[r * HD + lane + 64 * j] = (char)(int)q;
    if ((lane & 31) == 0) scales[r * (HD / 32) + (lane >> 5) + 2 * j] = dh;
  }
}

template <int HD>
static void launch_append_q8(const KvAppendQ8Args& a, dim3 grid, hipStream_t s) {
  if (a.qk_norm) hipLaunchKernelGGL((rope_kv_append_q8_kernel<HD, true, false>), grid, dim3(256), 0, s, a);
  else if (a.bias) hipLaunchKernelGGL((rope_kv_append_q8_kernel<HD, false, true>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((rope_kv_append_q8_kernel<HD, false, false>), grid, dim3(256), 0, s, a);
}

void rope_kv_append_q8(const KvAppendQ8Args& a, hipStream_t s) {
  if (a.T <= 0) return;
  if ((a.pos_arr == nullptr) != (a.slot_arr == nullptr)) throw std::runtime_error("rope_kv_append_q8: pos/slot arrays");
  if (a.head_dim != 64 && a.head_dim != 128) throw std::runtime_error("rope_kv_append_q8: head_dim must be 64 or 128");
  if (a.n_q % a.head_dim || a.n_kv % a.head_dim || a.n_kv < a.head_dim) throw std::runtime_error("rope_kv_append_q8: whole heads");
  if (a.qk_norm && a.bias) throw std::runtime_error("rope_kv_append_q8: no model has both QK-norm and Q|K|V biases");
  if (a.pos_dev && (a.pos_arr || a.T != 1)) throw std::runtime_error("rope_kv_append_q8: a device position serves one row");
  if (!a.pos_arr && !a.pos_dev && (a.pos0 < 0 || a.pos0 + a.T > a.n_ctx))
    throw std::runtime_error("rope_kv_append_q8: pos0 + T > n_ctx");
  const dim3 grid(a.T, ((a.n_q + 2 * a.n_kv) / a.head_dim + 3) / 4);
  if (a.head_dim == 128) launch_append_q8<128>(a, grid, s);
  else launch_append_q8<64>(a, grid, s);
}

// ---------------------------------------------------------------- decode
template <int HD, int G>
__global__ __launch_bounds__(256) void attn_decode_q8_kernel(AttnDecodeArgs a) {
  attn_decode_q8_body<HD, G>(a);
}

template <int HD>
static void launch_attn_decode_q8(const AttnDecodeArgs& a, int G, dim3 grid, hipStream_t s) {
  switch (G) {
    case 1: hipLaunchKernelGGL((attn_decode_q8_kernel<HD, 1>), grid, dim3(256), 0, s, a); break;
    case 2: hipLaunchKernelGGL((attn_decode_q8_kernel<HD, 2>), grid, dim3(256), 0, s, a); break;
    case 3: hipLaunchKernelGGL((attn_decode_q8_kernel<HD, 3>), grid, dim3(256), 0, s, a); break;
    case 4: hipLaunchKernelGGL((attn_decode_q8_kernel<HD, 4>), grid, dim3(256), 0, s, a); break;
    case 5: hipLaunchKernelGGL((attn_decode_q8_kernel<HD, 5>), grid, dim3(256), 0, s, a); break;
    case 6: hipLaunchKernelGGL((attn_decode_q8_kernel<HD, 6>), grid, dim3(256), 0, s, a); break;
    case 7: hipLaunchKernelGGL((attn_decode_q8_kernel<HD, 7>), grid, dim3(256), 0, s, a); break;
    case 8: hipLaunchKernelGGL((attn_decode_q8_kernel<HD, 8>), grid, dim3(256), 0, s, a); break;
    default: throw std::runtime_error("attn_decode_q8: gqa group must be 1 to 8");
  }
}

void attn_decode_q8(const AttnDecodeArgs& a, hipStream_t s) {
  if (a.n_kv_head < 1 || a.n_head % a.n_kv_head) throw std::runtime_error("attn_decode_q8: n_head % n_kv_head");
  if (!a.counters || !a.part || !a.pos) throw std::runtime_error("attn_decode_q8: workspaces missing");
  if (a.n_kv_head > 64) throw std::runtime_error("attn_decode_q8: at most 64 kv heads (split counters)");
  // the append kernel has finished the keys: no raw sums, biases, head norm, deferred rotation; no
  // in-launch consumer, weight touch or timeline either
  if (a.qkv_raw || a.qkv_bias || a.qk_norm || a.rope_freq || a.done || a.dbg_clk || a.live || a.debug_stop)
    throw std::runtime_error("attn_decode_q8: only the plain form (finished q, appended keys)");
  for (int r = 0; r < AttnDecodeArgs::kTouchRanges; ++r)
    if (a.pf[r]) throw std::runtime_error("attn_decode_q8: no weight touch");
  if (a.batch > 0 && (!a.slots || a.part_stride < attn_decode_workspace_floats(a.n_ctx, a.n_head, a.head_dim)))
    throw std::runtime_error("attn_decode_q8: bad batched arguments");
  const int G = a.n_head / a.n_kv_head;
  dim3 grid(a.n_kv_head, (a.n_ctx + CH - 1) / CH, a.batch > 0 ? a.batch : 1);
  if (a.head_dim == 128) launch_attn_decode_q8<128>(a, G, grid, s);
  else if (a.head_dim == 64) launch_attn_decode_q8<64>(a, G, grid, s);
  else throw std::runtime_error("attn_decode_q8: head_dim must be 64 or 128");
}

// ---------------------------------------------------------------- prefill on MFMA
// attention.hip's attn_prefill_mfma_kernel (block = one kv head x 4 waves, S^T = K . Q^T, online
// softmax per lane column, O^T += V^T . P^T with P^T in registers, the permuted key order, V^T through
// ds_read_b64_tr_b16) over a Q8_0 cache. Per 64-key tile a thread fetches HD / 64 16-byte int8 chunks
// of K and of V and each chunk's scale (a chunk is half a block); the next tile's chunks stay in
// flight in registers during the math, and each becomes 16 f16 values q * d on its way into Ks / Vs.
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef short s16x4_t __attribute__((ext_vector_type(4)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef float f32x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

// 16 int8 -> 16 f16 scaled by d, as two 16-byte LDS stores
__device__ __forceinline__ void q8_stage16(_Float16* dst, v4u raw, _Float16 d) {
  const h2v dd = {d, d};
  h2v p[8];
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    q8_cvt4(raw[w], p[2 * w], p[2 * w + 1]);
    p[2 * w] *= dd;
    p[2 * w + 1] *= dd;
  }
  const v4u lo = {__builtin_bit_cast(unsigned, p[0]), __builtin_bit_cast(unsigned, p[1]),
                  __builtin_bit_cast(unsigned, p[2]), __builtin_bit_cast(unsigned, p[3])};
  const v4u hi = {__builtin_bit_cast(unsigned, p[4]), __builtin_bit_cast(unsigned, p[5]),
                  __builtin_bit_cast(unsigned, p[6]), __builtin_bit_cast(unsigned, p[7])};
  *reinterpret_cast<v4u*>(dst) = lo;
  *reinterpret_cast<v4u*>(dst + 8) = hi;
}

// OUT: 0 f32, 1 bf16, 2 f16 in bmm's 4-group k order (gemm_t16's input)
template <int HD, int OUT>
__global__ __launch_bounds__(256) void attn_prefill_mfma_q8_kernel(AttnPrefillArgs a, int HB) {
  constexpr int KT = 64, KP = HD + 8, VP = HD + 32, NKK = HD / 16, NDT = HD / 32;
  constexpr int CPR = HD / 16, NCH = KT * CPR / 256, NB = HD / 32;  // 16-B int8 chunks per row / per thread
  __shared__ __attribute__((aligned(16))) _Float16 Ks[KT * KP];
  __shared__ __attribute__((aligned(16))) _Float16 Vs[KT * VP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 31, hh = lane >> 5;
  const int G = a.n_head / a.n_kv_head, QTB = 4 / HB;
  const int kvh = blockIdx.x;
  const int qblk = gridDim.y - 1 - blockIdx.y;  // latest (longest) query tiles dispatch first
  int T = a.T, pos0 = a.pos0, hz = blockIdx.z;
  size_t row0 = 0, cache0 = 0;  // cache0: bytes
  if (a.n_pieces > 0) {
    const int HZ = (G + HB - 1) / HB, pc = blockIdx.z / HZ;
    hz = blockIdx.z - pc * HZ;
    T = a.pc_n[pc];
    pos0 = a.pc_pos[pc];
    row0 = (size_t)a.pc_row[pc];
    cache0 = (size_t)a.pc_slot[pc] * a.slot_stride * sizeof(__half);
    if (qblk * QTB * 32 >= T) return;  // a shorter piece's missing tiles: whole block, no barrier yet
  }
  const int hl = hz * HB + wave % HB;
  const bool hreal = hl < G;
  const int head = kvh * G + min(hl, G - 1);
  const int tq = (qblk * QTB + wave / HB) * 32;
  const int nkeys = pos0 + min(T, (qblk + 1) * QTB * 32);  // keys the block needs
  const int wkeys = pos0 + min(T, tq + 32);                 // keys this wave needs
  const int t = tq + lr;
  const int qpos = pos0 + min(t, T - 1);  // padded query columns attend like the last real one

  f16x8_t qf[NKK];
  {
    const float* qr = a.q + ((row0 + min(t, T - 1)) * a.n_head + head) * HD + 8 * hh;
    const float qs = a.scale * 1.44269504088896341f;
    f32x4_t qv[2 * NKK];
#pragma unroll
    for (int i = 0; i < 2 * NKK; ++i) qv[i] = *reinterpret_cast<const f32x4_t*>(qr + 8 * (i >> 1) * 2 + 4 * (i & 1));
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk) {
      const f32x4_t v0 = qv[2 * kk], v1 = qv[2 * kk + 1];
      const f32x8_t v = {v0.x * qs, v0.y * qs, v0.z * qs, v0.w * qs, v1.x * qs, v1.y * qs, v1.z * qs, v1.w * qs};
      qf[kk] = __builtin_convertvector(v, f16x8_t);
    }
  }
  const char* kc = reinterpret_cast<const char*>(a.k_cache) + cache0;
  const char* vc = reinterpret_cast<const char*>(a.v_cache) + cache0;
  const _Float16* ksc = reinterpret_cast<const _Float16*>(kc + (size_t)a.n_kv_head * a.n_ctx * HD) + (size_t)kvh * a.n_ctx * NB;
  const _Float16* vsc = reinterpret_cast<const _Float16*>(vc + (size_t)a.n_kv_head * a.n_ctx * HD) + (size_t)kvh * a.n_ctx * NB;
  const char* kb = kc + (size_t)kvh * a.n_ctx * HD;
  const char* vb = vc + (size_t)kvh * a.n_ctx * HD;
  // rows clamped to the last needed key (written by the append before this launch): every load is
  // unconditional and no row past it - stale scales may be NaN - is ever read
  int goff[NCH], skey[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = tid + 256 * i;
    skey[i] = c / CPR;
    goff[i] = 16 * (c % CPR);
  }
  v4u kr[NCH], vr[NCH];
  _Float16 kd[NCH], vd[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const size_t row = (size_t)min(skey[i], nkeys - 1);
    kr[i] = *reinterpret_cast<const v4u*>(kb + row * HD + goff[i]);
    vr[i] = *reinterpret_cast<const v4u*>(vb + row * HD + goff[i]);
    kd[i] = ksc[row * NB + goff[i] / 32];
    vd[i] = vsc[row * NB + goff[i] / 32];
  }
  f32x16_t o[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
  float m = -1e30f, l = 0.f;
  const int trow = ((lane & 15) >> 2) + 4 * hh, tcol = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
  for (int k0 = 0; k0 < nkeys; k0 += KT) {
    __syncthreads();  // every wave is done with the previous tile
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      q8_stage16(Ks + skey[i] * KP + goff[i], kr[i], kd[i]);
      q8_stage16(Vs + skey[i] * VP + goff[i], vr[i], vd[i]);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NCH; ++i) {  // next tile in flight during this one's math (clamped on the last)
      const size_t row = (size_t)min(k0 + KT + skey[i], nkeys - 1);
      kr[i] = *reinterpret_cast<const v4u*>(kb + row * HD + goff[i]);
      vr[i] = *reinterpret_cast<const v4u*>(vb + row * HD + goff[i]);
      kd[i] = ksc[row * NB + goff[i] / 32];
      vd[i] = vsc[row * NB + goff[i] / 32];
    }
    if (k0 < wkeys) {  // wave-uniform: EXEC stays full for the transposed reads
      f32x16_t sc[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[j][r] = 0.f;
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) {
          const f16x8_t kv = *reinterpret_cast<const f16x8_t*>(Ks + (32 * j + lr) * KP + 16 * kk + 8 * hh);
          sc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kv, qf[kk], sc[j], 0, 0, 0);
        }
      }
      float mx = -INFINITY;
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = k0 + 32 * j + (r & 3) + 8 * (r >> 2) + 4 * hh;
          sc[j][r] = key <= qpos ? sc[j][r] : -INFINITY;
          mx = fmaxf(mx, sc[j][r]);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float mn = fmaxf(m, mx), alpha = exp2f(m - mn);
      m = mn;
      float ls = 0.f;
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          sc[j][r] = exp2f(sc[j][r] - mn);
          ls += sc[j][r];
        }
      l = l * alpha + ls;  // this half's keys; the halves are summed once at the end
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int hs = 0; hs < 2; ++hs) {
          const f32x8_t pv = {sc[j][8 * hs], sc[j][8 * hs + 1], sc[j][8 * hs + 2], sc[j][8 * hs + 3],
                              sc[j][8 * hs + 4], sc[j][8 * hs + 5], sc[j][8 * hs + 6], sc[j][8 * hs + 7]};
          const f16x8_t pb = __builtin_convertvector(pv, f16x8_t);
          const _Float16* vrow = Vs + (32 * j + 16 * hs + trow) * VP + tcol;
#pragma unroll
          for (int dt = 0; dt < NDT; ++dt) {
            typedef __attribute__((address_space(3))) s16x4_t lds_s16x4;
            const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(vrow + 32 * dt));
            const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(vrow + 8 * VP + 32 * dt));
            const f16x8_t va = __builtin_bit_cast(f16x8_t, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
            o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(va, pb, o[dt], 0, 0, 0);
          }
        }
    }
  }
  l += __shfl_xor(l, 32);
  const float inv = 1.f / l;
  if (t < T && hreal) {
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        const int d = 32 * dt + 8 * rg + 4 * hh;  // o[dt][4rg + 0..3] = dims d .. d+3
        const size_t off = (row0 + t) * a.out_stride + (size_t)head * HD + d;
        const float v0 = o[dt][4 * rg] * inv, v1 = o[dt][4 * rg + 1] * inv;
        const float v2 = o[dt][4 * rg + 2] * inv, v3 = o[dt][4 * rg + 3] * inv;
        if constexpr (OUT == 1) {
          const uint2 pk = make_uint2(pk_bf16_pair(v0, v1), pk_bf16_pair(v2, v3));
          *reinterpret_cast<uint2*>(a.out_bf16 + off) = pk;
        } else if constexpr (OUT == 2) {  // positions (0, 2, 1, 3) of the 4-group
          const __half2 p0 = __floats2half2_rn(v0, v2), p1 = __floats2half2_rn(v1, v3);
          *reinterpret_cast<uint2*>(a.out_h + off) =
              make_uint2(__builtin_bit_cast(unsigned, p0), __builtin_bit_cast(unsigned, p1));
        } else {
          *reinterpret_cast<float4*>(a.out + off) = make_float4(v0, v1, v2, v3);
        }
      }
  }
}

template <int HD>
static void launch_attn_prefill_q8(const AttnPrefillArgs& a, int G, hipStream_t s) {
  // heads per block as the f16 kernel: min(G, 4) for the power-of-two groups, else 4 with padded waves
  const int HB = (G & (G - 1)) == 0 ? std::min(G, 4) : 4, QTB = 4 / HB;
  int tmax = a.T;
  if (a.n_pieces > 0) {
    tmax = 0;
    for (int i = 0; i < a.n_pieces; ++i) tmax = std::max(tmax, a.pc_n[i]);
  }
  dim3 grid(a.n_kv_head, (tmax + 32 * QTB - 1) / (32 * QTB), ((G + HB - 1) / HB) * std::max(1, a.n_pieces));
  if (a.out_h) hipLaunchKernelGGL((attn_prefill_mfma_q8_kernel<HD, 2>), grid, dim3(256), 0, s, a, HB);
  else if (a.out_bf16) hipLaunchKernelGGL((attn_prefill_mfma_q8_kernel<HD, 1>), grid, dim3(256), 0, s, a, HB);
  else hipLaunchKernelGGL((attn_prefill_mfma_q8_kernel<HD, 0>), grid, dim3(256), 0, s, a, HB);
}

void attn_prefill_q8(const AttnPrefillArgs& a, hipStream_t s) {
  if (a.n_pieces < 0 || a.n_pieces > AttnPrefillArgs::kMaxPieces) throw std::runtime_error("attn_prefill_q8: 0-16 pieces");
  if (a.n_pieces > 0) {
    for (int i = 0; i < a.n_pieces; ++i)
      if (a.pc_n[i] <= 0 || a.pc_pos[i] < 0 || a.pc_pos[i] + a.pc_n[i] > a.n_ctx || a.pc_row[i] < 0 || a.pc_slot[i] < 0)
        throw std::runtime_error("attn_prefill_q8: bad piece");
  } else if (a.T <= 0) {
    return;
  }
  if (a.n_kv_head < 1 || a.n_head % a.n_kv_head) throw std::runtime_error("attn_prefill_q8: n_head % n_kv_head");
  if (a.head_dim != 128 && a.head_dim != 64) throw std::runtime_error("attn_prefill_q8: head_dim must be 64 or 128");
  if (a.n_pieces == 0 && (a.pos0 < 0 || a.pos0 + a.T > a.n_ctx)) throw std::runtime_error("attn_prefill_q8: pos0 + T > n_ctx");
  if (!a.out && !a.out_bf16 && !a.out_h) throw std::runtime_error("attn_prefill_q8: no output");
  const int G = a.n_head / a.n_kv_head;
  if (G > 16) throw std::runtime_error("attn_prefill_q8: gqa group must be 1 to 16");
  if (a.head_dim == 128) launch_attn_prefill_q8<128>(a, G, s);
  else launch_attn_prefill_q8<64>(a, G, s);
}

}  // namespace lfk
