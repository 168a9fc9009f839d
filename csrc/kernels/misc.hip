// Small kernels: embedding gather (on the GPU, not the CPU),
// RMSNorm->bf16 for the prefill GEMMs (K2), prefill RoPE + KV append (K5/K6),
// helpers, and the on-device synthetic weight generator.
#include <algorithm>
#include <stdexcept>
#include <hip/hip_bf16.h>

#include "kernels.h"
#include "qdot.h"

namespace lfk {

template <int QT>
__device__ void embed_row(const QMat& e, int token, int t, float* x) {
  // clamped: a token id can only come from the host (validated) or the sampler, but a
  // corrupted id must not turn into an out-of-bounds read that faults the GPU
  const size_t row = (size_t)min(max(token, 0), e.rows - 1);
  const int nq = e.K >> 5;
  for (int q = threadIdx.x; q < nq; q += blockDim.x) {
    float v[32];
    dequant32<QT>(e.base, e.P, row, q, v);
    float4* dst = reinterpret_cast<float4*>(x + (size_t)t * e.K + 32 * q);
#pragma unroll
    for (int i = 0; i < 8; ++i) dst[i] = make_float4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
  }
}
template <int QT>
__device__ void embed_body(const QMat& e, const int* tokens, int T, float* x) {
  embed_row<QT>(e, tokens[blockIdx.x], blockIdx.x, x);
}

// side job: zero [zero, zero + zero_n) ints (the decode step's done counters, attn_wo1)
__global__ __launch_bounds__(128) void embed_kernel(QMat e, const int* tokens, int T, float* x, int* zero, int zero_n) {
  for (int i = blockIdx.x * 128 + threadIdx.x; i < zero_n; i += gridDim.x * 128) zero[i] = 0;
  // wave-uniform; a type outside the list runs nothing here: embed_rows checks it and throws
  LFK_DISPATCH(LFK_TYPES_KERNEL, e.type, , embed_body<QT>(e, tokens, T, x));
}

void embed_rows(const QMat& emb, const int* tokens, int T, float* x, hipStream_t s, int* zero, int zero_n) {
  if (T <= 0) return;
  if (!dispatchable_type(emb.type)) throw std::runtime_error("embed_rows: unsupported embedding type");
  hipLaunchKernelGGL(embed_kernel, dim3(T), dim3(128), 0, s, emb, tokens, T, x, zero, zero ? zero_n : 0);
}

template <bool F16SW>
__global__ __launch_bounds__(256) void rmsnorm_bf16_kernel(const float* x, const float* w, float eps, int d,
                                                          __hip_bfloat16* y, float* zero, int zero_ld) {
  const int t = blockIdx.x, tid = threadIdx.x;
  const float* xr = x + (size_t)t * d;
  __shared__ float red[4];
  float ss = 0.f;
  for (int i = tid * 4; i < d; i += 1024) {
    float4 v = *reinterpret_cast<const float4*>(xr + i);
    ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
  if (zero) {  // the next GEMM's split-K partials meet in this row by atomic add
    float4* zr = reinterpret_cast<float4*>(zero + (size_t)t * zero_ld);
    for (int i = tid; i < zero_ld / 4; i += 256) zr[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  ss = wave_sum(ss);
  if ((tid & 63) == 0) red[tid >> 6] = ss;
  __syncthreads();
  const float sc = rsqrtf((red[0] + red[1] + red[2] + red[3]) / (float)d + eps);
  for (int i = tid * 4; i < d; i += 1024) {
    float4 v = *reinterpret_cast<const float4*>(xr + i);
    float4 g = *reinterpret_cast<const float4*>(w + i);
    if constexpr (F16SW) {  // 4-group order (0, 2, 1, 3): the pairs (0, 2) and (1, 3)
      const __half2 p0 = __floats2half2_rn(v.x * sc * g.x, v.z * sc * g.z);
      const __half2 p1 = __floats2half2_rn(v.y * sc * g.y, v.w * sc * g.w);
      *reinterpret_cast<uint2*>(y + (size_t)t * d + i) =
          make_uint2(__builtin_bit_cast(unsigned, p0), __builtin_bit_cast(unsigned, p1));
    } else {
      *reinterpret_cast<uint2*>(y + (size_t)t * d + i) =
          make_uint2(pk_bf16_pair(v.x * sc * g.x, v.y * sc * g.y), pk_bf16_pair(v.z * sc * g.z, v.w * sc * g.w));
    }
  }
}

void rmsnorm_bf16(const float* x, const float* w, float eps, int T, int d, __hip_bfloat16* y, hipStream_t s,
                  float* zero, int zero_ld, bool f16sw) {
  if (T <= 0) return;
  if (zero && (zero_ld % 4 || reinterpret_cast<uintptr_t>(zero) % 16))
    throw std::runtime_error("rmsnorm_bf16: zeroed rows must be float4 aligned");
  if (f16sw) hipLaunchKernelGGL(rmsnorm_bf16_kernel<true>, dim3(T), dim3(256), 0, s, x, w, eps, d, y, zero, zero_ld);
  else hipLaunchKernelGGL(rmsnorm_bf16_kernel<false>, dim3(T), dim3(256), 0, s, x, w, eps, d, y, zero, zero_ld);
}

__global__ void to_bf16_kernel(const float* x, int n, __hip_bfloat16* y) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = __float2bfloat16(x[i]);
}

void to_bf16(const float* x, int n, __hip_bfloat16* y, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(to_bf16_kernel, dim3((n + 255) / 256), dim3(256), 0, s, x, n, y);
}

// BIAS: Q|K|V biases [n_q + 2 n_kv] added before the rotation (qwen2; its own instantiation)
template <bool BIAS>
__global__ __launch_bounds__(256) void rope_kv_prefill_kernel(const float* qkv, int pos0, int n_q, int n_kv, int hd,
                                                              int n_ctx, const float2* rope, float* q_out,
                                                              __half* kc, __half* vc, const int* pos_arr,
                                                              const int* slot_arr, size_t slot_stride,
                                                              const float* bias) {
  const int t = blockIdx.x;
  const int pos = pos_arr ? min(max(pos_arr[t], 0), n_ctx - 1) : pos0 + t;
  if (slot_arr) {
    kc += (size_t)slot_arr[t] * slot_stride;
    vc += (size_t)slot_arr[t] * slot_stride;
  }
  const int ncol = n_q + 2 * n_kv;
  const float* row = qkv + (size_t)t * ncol;
  for (int p = threadIdx.x; p < ncol / 2; p += blockDim.x) {
    int c = 2 * p;
    float a0 = row[c], a1 = row[c + 1];
    if constexpr (BIAS) {
      a0 += bias[c];
      a1 += bias[c + 1];
    }
    if (c < n_q + n_kv) {
      const int dd = (c < n_q ? c : c - n_q) % hd;
      const float2 cs = rope[(size_t)pos * (hd >> 1) + (dd >> 1)];
      const float y0 = a0 * cs.x - a1 * cs.y, y1 = a0 * cs.y + a1 * cs.x;
      a0 = y0;
      a1 = y1;
    }
    if (c < n_q) {
      q_out[(size_t)t * n_q + c] = a0;
      q_out[(size_t)t * n_q + c + 1] = a1;
    } else {
      const bool isk = c < n_q + n_kv;
      const int r = isk ? c - n_q : c - n_q - n_kv;
      const int kvh = r / hd, dd = r % hd;
      __half* dst = (isk ? kc : vc) + ((size_t)kvh * n_ctx + pos) * hd + dd;
      dst[0] = __float2half(a0);
      dst[1] = __float2half(a1);
    }
  }
}

void rope_kv_prefill(const float* qkv, int T, int pos0, int n_q, int n_kv, int head_dim, int n_ctx, const float2* rope,
                     float* q_out, __half* k_cache, __half* v_cache, hipStream_t s, const int* pos_arr,
                     const int* slot_arr, size_t slot_stride, const float* bias) {
  if (T <= 0) return;
  if ((pos_arr == nullptr) != (slot_arr == nullptr)) throw std::runtime_error("rope_kv_prefill: pos/slot arrays");
  if (bias)
    hipLaunchKernelGGL(rope_kv_prefill_kernel<true>, dim3(T), dim3(256), 0, s, qkv, pos0, n_q, n_kv, head_dim, n_ctx,
                       rope, q_out, k_cache, v_cache, pos_arr, slot_arr, slot_stride, bias);
  else
    hipLaunchKernelGGL(rope_kv_prefill_kernel<false>, dim3(T), dim3(256), 0, s, qkv, pos0, n_q, n_kv, head_dim, n_ctx,
                       rope, q_out, k_cache, v_cache, pos_arr, slot_arr, slot_stride, bias);
}

// QK-norm models (qwen3): rope_kv_prefill with an RMSNorm over each q and k head in front of the
// rotation. One wave owns one head of one token (q heads, then k, then v): lane p holds the adjacent
// pair p of the head (HD 64: the lanes 32 .. 63 hold nothing), the head's sum of squares is a wave
// reduction. A kernel of its own beside rope_kv_prefill_kernel, which other models keep.
template <int HD>
__global__ __launch_bounds__(256) void qk_norm_rope_kv_kernel(const float* qkv, int pos0, int n_q, int n_kv, int n_ctx,
                                                              const float2* rope, const float* qk_norm, float eps,
                                                              float* q_out, __half* kc, __half* vc,
                                                              const int* pos_arr, const int* slot_arr,
                                                              size_t slot_stride, const int* pos_dev) {
  const int t = blockIdx.x, lane = threadIdx.x & 63;
  const int nhq = n_q / HD, nhk = n_kv / HD;
  const int h = blockIdx.y * 4 + (threadIdx.x >> 6);  // wave-uniform
  if (h >= nhq + 2 * nhk) return;
  const int pos = pos_arr ? min(max(pos_arr[t], 0), n_ctx - 1)
                          : pos_dev ? min(max(*pos_dev, 0), n_ctx - 1) : pos0 + t;
  if (slot_arr) {
    kc += (size_t)slot_arr[t] * slot_stride;
    vc += (size_t)slot_arr[t] * slot_stride;
  }
  const bool on = lane < HD / 2;
  const int p = on ? lane : 0;
  const float2 a = reinterpret_cast<const float2*>(qkv + (size_t)t * (n_q + 2 * n_kv) + (size_t)h * HD)[p];
  float y0 = a.x, y1 = a.y;
  if (h < nhq + nhk) {  // q or k: head norm, then the rotation
    const float2 w = reinterpret_cast<const float2*>(qk_norm + (h < nhq ? 0 : HD))[p];
    const float2 cs = rope[(size_t)pos * (HD / 2) + p];
    const float ss = wave_sum(on ? a.x * a.x + a.y * a.y : 0.f);
    const float sc = rsqrtf(ss * (1.f / HD) + eps);
    const float n0 = a.x * sc * w.x, n1 = a.y * sc * w.y;
    y0 = n0 * cs.x - n1 * cs.y;
    y1 = n0 * cs.y + n1 * cs.x;
  }
  if (!on) return;
  if (h < nhq) {
    reinterpret_cast<float2*>(q_out + (size_t)t * n_q + (size_t)h * HD)[p] = make_float2(y0, y1);
  } else {
    const bool isk = h < nhq + nhk;
    const int kvh = isk ? h - nhq : h - nhq - nhk;
    __half* dst = (isk ? kc : vc) + ((size_t)kvh * n_ctx + pos) * HD;
    reinterpret_cast<__half2*>(dst)[p] = __floats2half2_rn(y0, y1);
  }
}

void qk_norm_rope_kv(const float* qkv, int T, int pos0, int n_q, int n_kv, int head_dim, int n_ctx, const float2* rope,
                     const float* qk_norm, float eps, float* q_out, __half* k_cache, __half* v_cache, hipStream_t s,
                     const int* pos_arr, const int* slot_arr, size_t slot_stride, const int* pos_dev) {
  if (T <= 0) return;
  if ((pos_arr == nullptr) != (slot_arr == nullptr)) throw std::runtime_error("qk_norm_rope_kv: pos/slot arrays");
  if (!qk_norm) throw std::runtime_error("qk_norm_rope_kv: the norm weights are required");
  if (head_dim != 64 && head_dim != 128) throw std::runtime_error("qk_norm_rope_kv: head_dim must be 64 or 128");
  if (n_q % head_dim || n_kv % head_dim) throw std::runtime_error("qk_norm_rope_kv: whole heads");
  if (pos_dev && (pos_arr || T != 1)) throw std::runtime_error("qk_norm_rope_kv: a device position serves one row");
  if (!pos_arr && !pos_dev && (pos0 < 0 || pos0 + T > n_ctx)) throw std::runtime_error("qk_norm_rope_kv: pos0 + T > n_ctx");
  const dim3 grid(T, ((n_q + 2 * n_kv) / head_dim + 3) / 4);
  if (head_dim == 128)
    hipLaunchKernelGGL(qk_norm_rope_kv_kernel<128>, grid, dim3(256), 0, s, qkv, pos0, n_q, n_kv, n_ctx, rope, qk_norm,
                       eps, q_out, k_cache, v_cache, pos_arr, slot_arr, slot_stride, pos_dev);
  else
    hipLaunchKernelGGL(qk_norm_rope_kv_kernel<64>, grid, dim3(256), 0, s, qkv, pos0, n_q, n_kv, n_ctx, rope, qk_norm,
                       eps, q_out, k_cache, v_cache, pos_arr, slot_arr, slot_stride, pos_dev);
}

__global__ void batch_gather_kernel(const int* slots, int B, const int* state, int* tok, int* pos, int* zero,
                                    int zero_n, int zero_stride) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) {
    const int* st = state + (size_t)slots[b] * S_NSTATE;
    tok[b] = st[S_TOKEN];
    pos[b] = st[S_POS];
  }
  if (b < zero_n) zero[(size_t)b * zero_stride] = 0;
}
// (+ zero zero[i * zero_stride], i < zero_n: the step's in-launch chain counters)
void batch_gather(const int* slots, int B, const int* state, int* tok, int* pos, hipStream_t s, int* zero,
                  int zero_n, int zero_stride) {
  if (B <= 0) return;
  const int n = std::max(B, zero ? zero_n : 0);
  hipLaunchKernelGGL(batch_gather_kernel, dim3((n + 63) / 64), dim3(64), 0, s, slots, B, state, tok, pos, zero,
                     zero ? zero_n : 0, zero_stride);
}

// batched decode step head: block b gathers row b's token / position from its slot's state and
// embeds that token (one launch instead of batch_gather + embed_rows)
__global__ __launch_bounds__(128) void batch_embed_kernel(QMat e, const int* slots, const int* state, int* tok, int* pos,
                                                          float* x, int* zero, int zero_n, int zero_stride) {
  const int b = blockIdx.x;
  for (int i = b * 128 + threadIdx.x; i < zero_n; i += gridDim.x * 128) zero[(size_t)i * zero_stride] = 0;
  const int* st = state + (size_t)slots[b] * S_NSTATE;
  const int token = st[S_TOKEN];
  if (threadIdx.x == 0) {
    tok[b] = token;
    pos[b] = st[S_POS];
  }
  LFK_DISPATCH(LFK_TYPES_KERNEL, e.type, , embed_row<QT>(e, token, b, x));  // as embed_kernel
}
void batch_gather_embed(const int* slots, int B, const int* state, int* tok, int* pos, const QMat& emb, float* x,
                        hipStream_t s, int* zero, int zero_n, int zero_stride) {
  if (B <= 0) return;
  if (!dispatchable_type(emb.type)) throw std::runtime_error("batch_gather_embed: unsupported embedding type");
  hipLaunchKernelGGL(batch_embed_kernel, dim3(B), dim3(128), 0, s, emb, slots, state, tok, pos, x, zero,
                     zero ? zero_n : 0, zero_stride);
}

__global__ void add_inplace_kernel(float* x, const float* y, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) x[i] += y[i];
}
void add_inplace(float* x, const float* y, int n, hipStream_t s) {
  hipLaunchKernelGGL(add_inplace_kernel, dim3((n + 255) / 256), dim3(256), 0, s, x, y, n);
}

__global__ void set_i32_kernel(int* p, int v) { *p = v; }
void set_i32(int* p, int v, hipStream_t s) { hipLaunchKernelGGL(set_i32_kernel, dim3(1), dim3(1), 0, s, p, v); }

// ---------------------------------------------------------------- embedding epilogue (kernels.h PoolArgs)
// rsqrt(mean(x^2) + eps) of one row, by one wave (every lane returns it)
__device__ __forceinline__ float pool_row_scale(const float* xr, int d, float eps, int lane) {
  float ss = 0.f;
  for (int i = lane * 4; i < d; i += 256) {
    const float4 v = *reinterpret_cast<const float4*>(xr + i);
    ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
  return rsqrtf(wave_sum(ss) / (float)d + eps);
}

// block-wide sum of one value per thread (256 threads): waves in order, every thread returns it
__device__ __forceinline__ float pool_block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();  // (red may still be read from a previous call)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// the segment that block `b` of pool_rows works on and its group inside it; false: past the table
__device__ __forceinline__ bool pool_find(const int* segs, int n_segs, int mode, int b, int* seg, int* grp) {
  for (int k = 0; k < n_segs; ++k) {
    const int n = segs[k * kPoolSegInts + 1];
    const int g = mode == POOL_CLS || mode == POOL_LAST ? 1 : (n + kPoolGroup - 1) / kPoolGroup;
    if (b < g) {
      *seg = k;
      *grp = b;
      return true;
    }
    b -= g;
  }
  return false;
}

__global__ __launch_bounds__(256) void pool_rows_kernel(const float* x, int ldx, const float* w, float eps, int d,
                                                        int mode, int normalize, const int* segs, int n_segs,
                                                        float* part, float* out) {
  __shared__ float scale[kPoolGroup];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int k, g;
  if (!pool_find(segs, n_segs, mode, blockIdx.x, &k, &g)) return;  // block-uniform
  const int* sg = segs + k * kPoolSegInts;
  const int row0 = sg[0], n = sg[1], flags = sg[3];
  if (mode == POOL_NONE) {
    // a wave owns a row: normed, and divided by its own L2 norm if asked
    for (int r = g * kPoolGroup + wave; r < min(n, (g + 1) * kPoolGroup); r += 4) {
      const float* xr = x + (size_t)(row0 + r) * ldx;
      float* o = out + (size_t)(row0 + r) * d;
      const float sc = pool_row_scale(xr, d, eps, lane);
      float rn = 1.f;
      if (normalize) {
        float ss = 0.f;
        for (int i = lane * 4; i < d; i += 256) {
          const float4 v = *reinterpret_cast<const float4*>(xr + i);
          const float4 q = *reinterpret_cast<const float4*>(w + i);
          const float a = sc * v.x * q.x, b = sc * v.y * q.y, c = sc * v.z * q.z, e = sc * v.w * q.w;
          ss += a * a + b * b + c * c + e * e;
        }
        ss = wave_sum(ss);
        rn = ss > 0.f ? rsqrtf(ss) : 0.f;  // a zero row stays zero (upstream: norm > 0 ? 1 / norm : 0)
      }
      for (int i = lane * 4; i < d; i += 256) {
        const float4 v = *reinterpret_cast<const float4*>(xr + i);
        const float4 q = *reinterpret_cast<const float4*>(w + i);
        *reinterpret_cast<float4*>(o + i) =
            make_float4(sc * v.x * q.x * rn, sc * v.y * q.y * rn, sc * v.z * q.z * rn, sc * v.w * q.w * rn);
      }
    }
    return;
  }
  int r0, nr;  // the block's rows of the segment
  if (mode == POOL_MEAN) {
    r0 = g * kPoolGroup;
    nr = min(kPoolGroup, n - r0);
  } else {  // the input's first / last row, when this piece holds it
    if (!(flags & (mode == POOL_CLS ? kPoolFirst : kPoolLast))) return;
    r0 = mode == POOL_CLS ? 0 : n - 1;
    nr = 1;
  }
  const float* xg = x + (size_t)(row0 + r0) * ldx;
  for (int r = wave; r < nr; r += 4) {  // rows round-robin over the waves
    const float sc = pool_row_scale(xg + (size_t)r * ldx, d, eps, lane);
    if (lane == 0) scale[r] = sc;
  }
  __syncthreads();
  // partial row of the group: a segment's groups come first to last, the segments in table order
  int prow = g;
  for (int j = 0; j < k; ++j)
    prow += mode == POOL_MEAN ? (segs[j * kPoolSegInts + 1] + kPoolGroup - 1) / kPoolGroup : 1;
  float* p = part + (size_t)prow * d;
  for (int i = tid * 4; i < d; i += 1024) {  // a thread owns its columns; rows added in row order
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int r = 0; r < nr; ++r) {
      const float4 v = *reinterpret_cast<const float4*>(xg + (size_t)r * ldx + i);
      const float sc = scale[r];
      a.x += sc * v.x; a.y += sc * v.y; a.z += sc * v.z; a.w += sc * v.w;
    }
    const float4 q = *reinterpret_cast<const float4*>(w + i);
    *reinterpret_cast<float4*>(p + i) = make_float4(a.x * q.x, a.y * q.y, a.z * q.z, a.w * q.w);
  }
}

__global__ __launch_bounds__(256) void pool_finish_kernel(int d, int mode, int normalize, const int* segs, int n_segs,
                                                          const float* part, float* acc, float* out) {
  __shared__ float red[4];
  const int input = blockIdx.x, tid = threadIdx.x;
  // the input's segment of this launch (at most one: pool_part_rows checks) and its partial rows
  int k = -1, prow = 0;
  for (int j = 0; j < n_segs; ++j) {
    if (segs[j * kPoolSegInts + 2] == input) {
      k = j;
      break;
    }
    prow += mode == POOL_MEAN ? (segs[j * kPoolSegInts + 1] + kPoolGroup - 1) / kPoolGroup : 1;
  }
  if (k < 0) return;  // block-uniform: no piece of this input here, its rows stay
  const int* sg = segs + k * kPoolSegInts;
  const int n = sg[1], flags = sg[3], n_tokens = sg[4];
  int ng = (n + kPoolGroup - 1) / kPoolGroup;
  if (mode != POOL_MEAN) ng = (flags & (mode == POOL_CLS ? kPoolFirst : kPoolLast)) ? 1 : 0;
  const bool first = flags & kPoolFirst, last = flags & kPoolLast;
  const float inv_n = mode == POOL_MEAN ? 1.f / (float)n_tokens : 1.f;
  float* ar = acc + (size_t)input * d;
  float ss = 0.f;
  for (int i = tid * 4; i < d; i += 1024) {
    float4 a = first ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<const float4*>(ar + i);
    for (int j = 0; j < ng; ++j) {  // group order
      const float4 v = *reinterpret_cast<const float4*>(part + (size_t)(prow + j) * d + i);
      a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
    *reinterpret_cast<float4*>(ar + i) = a;
    a.x *= inv_n; a.y *= inv_n; a.z *= inv_n; a.w *= inv_n;
    ss += a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w;
  }
  if (!last) return;
  float rn = 1.f;
  if (normalize) {  // a zero vector stays zero (upstream: norm > 0 ? 1 / norm : 0)
    ss = pool_block_sum(ss, red);
    rn = ss > 0.f ? rsqrtf(ss) : 0.f;
  }
  for (int i = tid * 4; i < d; i += 1024) {  // (each thread re-reads the accumulator columns it wrote)
    const float4 a = *reinterpret_cast<const float4*>(ar + i);
    *reinterpret_cast<float4*>(out + (size_t)input * d + i) =
        make_float4(a.x * inv_n * rn, a.y * inv_n * rn, a.z * inv_n * rn, a.w * inv_n * rn);
  }
}

int pool_part_rows(const PoolArgs& a) {
  if (a.mode < POOL_NONE || a.mode > POOL_LAST) throw std::runtime_error("pool: unknown pooling mode");
  if (a.d < 4 || a.d % 4 || a.d > kPoolMaxD) throw std::runtime_error("pool: d must be a multiple of 4 up to 16384");
  if (a.ldx < a.d || a.ldx % 4) throw std::runtime_error("pool: ldx must be a multiple of 4, at least d");
  if (!a.x || !a.w || !a.segs || !a.h_segs || a.n_segs < 1) throw std::runtime_error("pool: missing arguments");
  if (reinterpret_cast<uintptr_t>(a.x) % 16 || reinterpret_cast<uintptr_t>(a.w) % 16 ||
      reinterpret_cast<uintptr_t>(a.part) % 16 || reinterpret_cast<uintptr_t>(a.acc) % 16 ||
      reinterpret_cast<uintptr_t>(a.out) % 16)
    throw std::runtime_error("pool: buffers must be 16-byte aligned");
  if (!a.out || (a.mode != POOL_NONE && (!a.part || !a.acc))) throw std::runtime_error("pool: missing buffers");
  int need = 0;
  for (int k = 0; k < a.n_segs; ++k) {
    const int* g = a.h_segs + k * kPoolSegInts;
    if (g[0] < 0 || g[1] < 1 || (long long)g[0] + g[1] > a.rows) throw std::runtime_error("pool: segment outside the rows");
    if (a.mode != POOL_NONE && (g[2] < 0 || g[2] >= a.n_inputs)) throw std::runtime_error("pool: input index out of range");
    if (g[3] & ~(kPoolFirst | kPoolLast)) throw std::runtime_error("pool: unknown segment flags");
    if (g[4] < g[1]) throw std::runtime_error("pool: a segment longer than its input");
    for (int j = 0; j < k; ++j)
      if (a.h_segs[j * kPoolSegInts + 2] == g[2]) throw std::runtime_error("pool: one segment per input and launch");
    need += a.mode == POOL_MEAN ? (g[1] + kPoolGroup - 1) / kPoolGroup : a.mode == POOL_NONE ? 0 : 1;
  }
  if (need > a.part_rows) throw std::runtime_error("pool: partial buffer too small");
  return need;
}

void pool_rows(const PoolArgs& a, hipStream_t s) {
  (void)pool_part_rows(a);
  int blocks = 0;
  for (int k = 0; k < a.n_segs; ++k) {
    const int n = a.h_segs[k * kPoolSegInts + 1];
    blocks += a.mode == POOL_CLS || a.mode == POOL_LAST ? 1 : (n + kPoolGroup - 1) / kPoolGroup;
  }
  hipLaunchKernelGGL(pool_rows_kernel, dim3(blocks), dim3(256), 0, s, a.x, a.ldx, a.w, a.eps, a.d, a.mode,
                     (int)a.normalize, a.segs, a.n_segs, a.part, a.out);
}

void pool_finish(const PoolArgs& a, hipStream_t s) {
  (void)pool_part_rows(a);
  if (a.mode == POOL_NONE) return;  // pool_rows wrote the rows
  hipLaunchKernelGGL(pool_finish_kernel, dim3(a.n_inputs), dim3(256), 0, s, a.d, a.mode, (int)a.normalize, a.segs,
                     a.n_segs, a.part, a.acc, a.out);
}

// ---------------------------------------------------------------- synthetic weights on device
__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__global__ void fill_bytes_kernel(uint32_t* p, size_t nwords, unsigned long long seed) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < nwords; i += (size_t)gridDim.x * blockDim.x)
    p[i] = (uint32_t)mix64(seed ^ (i * 0xD1B54A32D192ED03ull));
}

__device__ __forceinline__ float u01(unsigned long long h) { return (float)(h >> 40) * (1.f / 16777216.f); }

// Overwrite the scale fields of each block with finite values matching gguf/quants.py:random_blocks.
__global__ void fix_scales_kernel(uint8_t* base, int type, size_t nblocks, Planes P, float std, unsigned long long seed) {
  for (size_t b = blockIdx.x * (size_t)blockDim.x + threadIdx.x; b < nblocks; b += (size_t)gridDim.x * blockDim.x) {
    const float jit = 0.5f + u01(mix64(seed * 31 + b));
    if (type == T_Q4_K || type == T_Q5_K) {
      const float nmax = type == T_Q4_K ? 15.f : 31.f;
      const float var_sq = (63.f * 127.f / 6.f) * (nmax * (2.f * nmax + 1.f) / 6.f) - (31.5f * nmax / 2.f) * (31.5f * nmax / 2.f);
      const float var = var_sq + (nmax / 2.f) * (nmax / 2.f) * (64.f * 64.f - 1.f) / 12.f;
      const float d = std / sqrtf(var) * jit;
      // meta record b (16 B): d, dmin
      uint8_t* meta = base + (type == T_Q4_K ? P.p1 : P.p2) + 16 * b;
      reinterpret_cast<__half*>(meta)[0] = __float2half(d);
      reinterpret_cast<__half*>(meta)[1] = __float2half(d * nmax * 0.5f);
    } else if (type == T_Q6_K) {
      reinterpret_cast<__half*>(base + P.p3)[b] = __float2half(std / (73.9f * 18.5f) * jit);
    } else if (type == T_Q8_0) {
      reinterpret_cast<__half*>(base + P.p1)[b] = __float2half(std / 73.9f * jit);
    } else if (type == T_Q4_0 || type == T_Q4_1 || type == T_Q5_0 || type == T_Q5_1) {
      // q uniform in [0, nmax]; the -8 / -16 offset or m = -d nmax / 2 centres the weights
      const float nmax = (type == T_Q4_0 || type == T_Q4_1) ? 15.f : 31.f;
      const __half d = __float2half(std / sqrtf(((nmax + 1.f) * (nmax + 1.f) - 1.f) / 12.f) * jit);
      uint8_t* sp = base + ((type == T_Q4_0 || type == T_Q4_1) ? P.p1 : P.p2);
      if (type == T_Q4_0 || type == T_Q5_0) {
        reinterpret_cast<__half*>(sp)[b] = d;
      } else {
        reinterpret_cast<__half*>(sp)[2 * b] = d;
        reinterpret_cast<__half*>(sp)[2 * b + 1] = __float2half(-__half2float(d) * nmax * 0.5f);
      }
    } else if (type == T_Q2_K) {
      // sc, m uniform in [0, 15], q in [0, 3], dmin = 1.5 d centres the weights (random_blocks)
      const float var = (15.f * 31.f / 6.f) * 3.5f - (7.5f * 1.5f) * (7.5f * 1.5f) + 2.25f * (16.f * 16.f - 1.f) / 12.f;
      const float d = std / sqrtf(var) * jit;
      reinterpret_cast<__half*>(base + P.p2)[2 * b] = __float2half(d);
      reinterpret_cast<__half*>(base + P.p2)[2 * b + 1] = __float2half(d * 1.5f);
    } else if (type == T_Q3_K) {
      // sc - 32 uniform in [-32, 31] (mean square 341.5), q - 4 in [-4, 3] (mean square 5.5)
      reinterpret_cast<__half*>(base + P.p3)[b] = __float2half(std / sqrtf(341.5f * 5.5f) * jit);
    } else if (type == T_IQ4_NL) {
      // codebook index uniform (mean square 4548); a random sign of d centres the weights (the
      // codebook's mean is -5.875), as random_blocks
      const float sgn = (mix64(seed * 17 + b) & 1ull) ? 1.f : -1.f;
      reinterpret_cast<__half*>(base + P.p1)[b] = __float2half(sgn * std / sqrtf(4548.f) * jit);
    } else if (type == T_IQ4_XS) {
      // ls - 32 uniform in [-32, 31] (mean square 341.5); sc record b (8 B): d first
      reinterpret_cast<__half*>(base + P.p1 + 8 * b)[0] = __float2half(std / sqrtf(341.5f * 4548.f) * jit);
    } else if (type == T_F32) {
      // uniform in [-sqrt(3) std, sqrt(3) std]
      const float u = u01(mix64(seed ^ (b * 0x9E37ull)));
      reinterpret_cast<float*>(base)[b] = (2.f * u - 1.f) * 1.7320508f * std;
    } else if (type == T_F16) {
      const float u = u01(mix64(seed ^ (b * 0x9E37ull)));
      reinterpret_cast<__half*>(base)[b] = __float2half((2.f * u - 1.f) * 1.7320508f * std);
    }
  }
}

void fill_random_planar(uint8_t* base, int type, size_t rows, size_t K, float std, unsigned long long seed,
                        hipStream_t s) {
  const size_t bytes = qbytes(type, rows, K);
  const Planes P = planes_of(type, rows, K);
  hipLaunchKernelGGL(fill_bytes_kernel, dim3(2048), dim3(256), 0, s, reinterpret_cast<uint32_t*>(base), bytes / 4, seed);
  const size_t nblocks = rows * (K / type_info(type).block);  // qbytes above has refused an unknown type
  hipLaunchKernelGGL(fix_scales_kernel, dim3(2048), dim3(256), 0, s, base, type, nblocks, P, std, seed + 1);
}

}  // namespace lfk

namespace lfk {
// Clock probe (microbenchmarks): a dependent FMA chain timed in shader cycles
// (clock64) and in constant-rate wall ticks (wall_clock64, 100 MHz), so the
// ratio gives the shader clock the GPU actually ran at.
__global__ void clock_probe_kernel(long long* out, int iters) {
  const long long w0 = wall_clock64(), c0 = clock64();
  float x = threadIdx.x * 1e-3f;
  for (int i = 0; i < iters; ++i) x = fmaf(x, 0.999f, 0.5f);
  const long long c1 = clock64(), w1 = wall_clock64();
  if (threadIdx.x == 0) {
    out[0] = c1 - c0;
    out[1] = w1 - w0;
    out[2] = (long long)x;
  }
}
void clock_probe(long long* out, int iters, hipStream_t s) {
  hipLaunchKernelGGL(clock_probe_kernel, dim3(1), dim3(64), 0, s, out, iters);
}
}  // namespace lfk

namespace lfk {
// ---------------------------------------------------------------- launch-shape probe (microbenchmarks)
// A trivial kernel of the given geometry: every thread spins `iters` dependent
// FMAs, one lane per block writes. Timing a graph chain of these separates the
// per-launch cost of a workgroup shape (256 vs 1024 threads, LDS request) from
// any real kernel body.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void launch_probe_kernel(float* out, int iters) {
  extern __shared__ float lds_probe[];
  float v = (float)threadIdx.x;
  for (int i = 0; i < iters; ++i) v = v * 0.999f + 0.5f;
  if (threadIdx.x == 0) {
    lds_probe[0] = v;
    out[blockIdx.x & 1023] = lds_probe[0];
  }
}
void launch_probe(int threads, int blocks, size_t lds, int iters, float* out, hipStream_t s) {
  if (threads == 1024) hipLaunchKernelGGL(launch_probe_kernel<1024>, dim3(blocks), dim3(1024), lds, s, out, iters);
  else if (threads == 512) hipLaunchKernelGGL(launch_probe_kernel<512>, dim3(blocks), dim3(512), lds, s, out, iters);
  else hipLaunchKernelGGL(launch_probe_kernel<256>, dim3(blocks), dim3(256), lds, s, out, iters);
}
}  // namespace lfk
