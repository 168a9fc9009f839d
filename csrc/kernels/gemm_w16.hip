// GEMM for BF16 weights, no dequantisation (gemm_dq's contract, reached through gemm_dq):
//   Y[T][N] = X[T][K] (bf16) . W[N][K]^T (bf16, row-major)
//
// The weights already are the MFMA operand, so the weight path has no VALU instruction at all:
// HBM -> 16-byte loads -> ds_write_b128 -> ds_read_b128 -> MFMA, every byte unchanged.
//
// Work split. A 256-thread block (4 waves) owns a BMT (tokens) x BNT (weight rows) tile and walks
// K in 64-deep steps; one step of one weight row is exactly one 128-byte line.
//   * loads: thread i of a step's load j takes 16 B number (i & 7) of row (i + 256 j) >> 3, so
//     every load instruction of a wave reads 8 whole lines (8 lanes x 16 B per row). The MFMA
//     fragment map would give 2 (32x32x16) or 4 (16x16x32) lanes per row, half lines at best;
//     the transposition to the fragment map is what the LDS round trip is for.
//   * registers, not the global-to-LDS DMA: the loads of steps k+1 .. k+D sit in a D-deep
//     register ring (named stages, no private memory), so D - 1 steps are still in flight when a
//     stage's ds_write waits for it, while LDS holds two (double buffer, one barrier per step). With the DMA loads every step in flight needs its own LDS tile (D + 1
//     tiles, fewer blocks per CU), and its LDS rows cannot be padded: the 16-byte units of a wave
//     land back to back, which puts the fragment reads of 8 rows in the same banks. Rows here are
//     padded by 16 B (pitch 144 B), as gemm_dq's. What the DMA saves is the ds_write, which is no
//     bound here: a step costs 1-4 ds_write_b128 per thread beside 2-16 MFMAs.
//   * wide regime (prompt chunks, BMT = 64 / 128, BNT = 128): v_mfma_f32_32x32x16_bf16 with x as
//     A and the weights as B; wave w owns weight rows 32w .. 32w+31 and all BMT tokens.
//   * narrow regime (the batched step's 1-16 rows, BMT = 16, BNT = 64): a 64-token tile would
//     leave 3/4 of the matrix core idle and the launch is a pure weight stream, so the weights
//     are the A operand of v_mfma_f32_16x16x32_bf16 (16 rows per wave) and the <= 16 rows of x
//     the B operand; weight loads are non-temporal (read once per step), the ring is one deeper,
//     and K is split until ~4 blocks (16 waves, 4 per SIMD) per CU stream.
// Split-K partial tiles meet by atomic add (STORE: `out` zeroed first, by a kernel - a memset
// node does not belong in a captured graph). Ragged N and T: loads are clamped to the last row
// (an output depends on its own token row and weight row only, so a clamped row's products land
// in outputs that are not stored), stores are guarded. K % 64 == 0.
#include <hip/hip_bf16.h>

#include <algorithm>

#include "kernels.h"
#include "qdot.h"

namespace lfk {

typedef __attribute__((ext_vector_type(8))) short w16_bf16x8;
typedef __attribute__((ext_vector_type(8))) __bf16 w16_bf16x8n;
typedef __attribute__((ext_vector_type(4))) float w16_f32x4;
typedef __attribute__((ext_vector_type(16))) float w16_f32x16;

static constexpr int W16_BK = 64, W16_PITCH = W16_BK + 8;  // bf16 elements

template <int EPI, int BMT>
__global__ __launch_bounds__(256) void gemm_bf16w_kernel(GemmArgs a) {
  constexpr bool NARROW = BMT == 16;
  constexpr int BNT = NARROW ? 64 : 128, NT = 256, BK = W16_BK, PITCH = W16_PITCH;
  constexpr int D = NARROW ? 4 : 3;                          // register ring depth (K steps in flight)
  constexpr int WL = BNT * 8 / NT;                           // 16-B weight loads per thread per step
  constexpr int XL = (BMT * 8 + NT - 1) / NT;                // 16-B x loads (narrow: threads 0..127 only)
  constexpr int MT = NARROW ? 1 : BMT / 32;
  __shared__ __attribute__((aligned(16))) unsigned short lds[2 * (BMT + BNT) * PITCH];
  auto Xs = [&](int b) { return lds + b * BMT * PITCH; };
  auto Ws = [&](int b) { return lds + 2 * BMT * PITCH + b * BNT * PITCH; };
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * BNT, m0 = blockIdx.y * BMT;
  const int N = a.w.rows, K = a.w.K, T = a.T;
  const int nk = K / BK, ks = (nk + gridDim.z - 1) / gridDim.z;
  const int kb = blockIdx.z * ks, ke = min(nk, kb + ks);

  // this thread's 16-B units of a step: unit u = tid + NT i -> row u >> 3, k offset 8 (u & 7)
  const unsigned short* wg = reinterpret_cast<const unsigned short*>(a.w.base);
  const unsigned short* xg = reinterpret_cast<const unsigned short*>(a.x);
  const unsigned short* wp[WL];
  const unsigned short* xp[XL];
  const bool xload = !NARROW || tid < BMT * 8;
#pragma unroll
  for (int i = 0; i < WL; ++i) {
    const int u = tid + NT * i;
    wp[i] = wg + (size_t)min(n0 + (u >> 3), N - 1) * K + 8 * (u & 7);
  }
#pragma unroll
  for (int i = 0; i < XL; ++i) {
    const int u = NARROW ? (tid & (BMT * 8 - 1)) : tid + NT * i;
    xp[i] = xg + (size_t)min(m0 + (u >> 3), T - 1) * K + 8 * (u & 7);
  }
  // The ring's stages are named structs handed to the step by reference, so each one is a fixed set
  // of VGPRs: no private memory, and the only vmcnt waits are the ones in front of a stage's
  // ds_write. Every load is unconditional (the step clamped to the part's last): a load under a
  // runtime branch makes the compiler drain vmcnt at the join, which would serialise the ring.
  // (i32x4_t, the native vector: a copy of HIP's int4 struct is a memcpy the compiler does not split)
  struct Stage {
    i32x4_t w[WL], x[XL];
  };
  auto load_step = [&](Stage& st, int k) {
    const int k0 = min(k, ke - 1) * BK;
#pragma unroll
    for (int i = 0; i < XL; ++i) st.x[i] = *reinterpret_cast<const i32x4_t*>(xp[i] + k0);
#pragma unroll
    for (int i = 0; i < WL; ++i) {
      if constexpr (NARROW) st.w[i] = __builtin_nontemporal_load(reinterpret_cast<const i32x4_t*>(wp[i] + k0));
      else st.w[i] = *reinterpret_cast<const i32x4_t*>(wp[i] + k0);
    }
  };
  auto store_step = [&](const Stage& st, int buf) {
    if (xload) {
#pragma unroll
      for (int i = 0; i < XL; ++i) {
        const int u = tid + NT * i;
        *reinterpret_cast<i32x4_t*>(Xs(buf) + (u >> 3) * PITCH + 8 * (u & 7)) = st.x[i];
      }
    }
#pragma unroll
    for (int i = 0; i < WL; ++i) {
      const int u = tid + NT * i;
      *reinterpret_cast<i32x4_t*>(Ws(buf) + (u >> 3) * PITCH + 8 * (u & 7)) = st.w[i];
    }
  };

  w16_f32x16 acc[MT];   // wide
  w16_f32x4 acc4 = {0.f, 0.f, 0.f, 0.f};  // narrow
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;

  // one K step: `cur` held step k, already in LDS - refill it with step k + D (clamped past ke);
  // run step k's MFMAs from its LDS buffer; then move `nxt` (step k + 1) into the other buffer,
  // which was last read at step k - 1, behind that step's barrier
  auto step = [&](Stage& cur, const Stage& nxt, int k) {
    load_step(cur, k + D);
    if (k >= ke) return;
    const int buf = (k - kb) & 1;
    if constexpr (NARROW) {
      const int fr = lane & 15, fk = 8 * (lane >> 4);
#pragma unroll
      for (int kk = 0; kk < BK; kk += 32) {
        const w16_bf16x8n aw =
            *reinterpret_cast<const w16_bf16x8n*>(Ws(buf) + (16 * wave + fr) * PITCH + kk + fk);
        const w16_bf16x8n xb = *reinterpret_cast<const w16_bf16x8n*>(Xs(buf) + fr * PITCH + kk + fk);
        acc4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aw, xb, acc4, 0, 0, 0);
      }
    } else {
      const int lr = lane & 31, lk = 8 * (lane >> 5);
#pragma unroll
      for (int kk = 0; kk < BK; kk += 16) {
        const w16_bf16x8 bw = *reinterpret_cast<const w16_bf16x8*>(Ws(buf) + (32 * wave + lr) * PITCH + kk + lk);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          const w16_bf16x8 xv = *reinterpret_cast<const w16_bf16x8*>(Xs(buf) + (32 * m + lr) * PITCH + kk + lk);
          acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xv, bw, acc[m], 0, 0, 0);
        }
      }
    }
    if (k + 1 < ke) store_step(nxt, buf ^ 1);
    __syncthreads();
  };

  Stage s0, s1, s2, s3;  // (s3: the narrow regime's fourth stage)
  if (kb < ke) {
    load_step(s0, kb);
    load_step(s1, kb + 1);
    load_step(s2, kb + 2);
    if constexpr (D == 4) load_step(s3, kb + 3);
    store_step(s0, 0);
  }
  __syncthreads();
  for (int k = kb; k < ke; k += D) {
    step(s0, s1, k);
    step(s1, s2, k + 1);
    if constexpr (D == 4) {
      step(s2, s3, k + 2);
      step(s3, s0, k + 3);
    } else {
      step(s2, s0, k + 2);
    }
  }

  // ---- epilogue. Output element e of this lane: token te(e), column (weight row) ce(e).
  //   wide  : acc[m][r]: token 32m + (r&3) + 8(r>>2) + 4(lane>>5), column 32 wave + (lane&31)
  //   narrow: acc4[i]  : token lane & 15, column 16 wave + 4 (lane>>4) + i
  constexpr int NE = NARROW ? 4 : 16 * MT;
  auto val = [&](int e) { return NARROW ? acc4[e & 3] : acc[(e >> 4) % MT][e & 15]; };
  auto te = [&](int e) {
    if constexpr (NARROW) return m0 + (lane & 15);
    else return m0 + 32 * (e >> 4) + (e & 3) + 8 * ((e & 15) >> 2) + 4 * (lane >> 5);
  };
  auto ce = [&](int e) {  // column inside the block's tile
    if constexpr (NARROW) return 16 * wave + 4 * (lane >> 4) + e;
    else return 32 * wave + (lane & 31);
  };
  if constexpr (EPI == GEMM_SWIGLU) {
    // gate rows 64g .. 64g+31, up rows 64g+32 .. 64g+63: the up half's sums go through LDS to the
    // lanes that hold the gate sums of the same (token, feature). Wide: the odd waves hold up rows
    // (a 128-row tile is two groups); narrow: waves 2, 3 (the 64-row tile is one group).
    static_assert(2 * NE * 64 * 4 <= (int)sizeof(lds), "SwiGLU exchange does not fit");
    float* ex = reinterpret_cast<float*>(lds);
    const bool up = NARROW ? wave >= 2 : (wave & 1);
    const int pw = NARROW ? (wave & 1) : (wave >> 1);  // pair index of the wave
    __syncthreads();  // (the loop's last barrier already closed the tile reads; kept for the empty split)
    if (up) {
#pragma unroll
      for (int e = 0; e < NE; ++e) ex[(pw * NE + e) * 64 + lane] = val(e);
    }
    __syncthreads();
    if (!up) {
      const int F = N >> 1;
#pragma unroll
      for (int e = 0; e < NE; ++e) {
        const int c = n0 + ce(e), t = te(e);
        const int feat = (c >> 6) * 32 + (c & 31);
        if (t < T && feat < F) {
          const float g = val(e), u = ex[(pw * NE + e) * 64 + lane];
          a.out_bf16[(size_t)t * F + feat] = __float2bfloat16(g / (1.f + __expf(-g)) * u);
        }
      }
    }
  } else {
    if (kb >= ke) return;  // an empty K part adds nothing
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      const int c = n0 + ce(e), t = te(e);
      if (t < T && c < N) {
        float* o = a.out + (size_t)t * a.ldo + c;
        if (gridDim.z > 1) {  // split-K: partial tiles meet by atomic add (STORE outputs pre-zeroed)
          float v = val(e);
          if (EPI == GEMM_STORE && a.resid && blockIdx.z == 0) v += a.resid[(size_t)t * a.ldo + c];
          atomicAdd(o, v);
        } else if constexpr (EPI == GEMM_ADD) {
          *o += val(e);
        } else {
          *o = a.resid ? val(e) + a.resid[(size_t)t * a.ldo + c] : val(e);
        }
      }
    }
  }
}

// out[t][0 .. n) = 0 for t < T (row stride ldo): the split-K STORE's start value
__global__ __launch_bounds__(256) void gemm_bf16w_zero_kernel(float* out, int ldo, int n) {
  float* row = out + (size_t)blockIdx.x * ldo;
  for (int i = threadIdx.x; i < n; i += 256) row[i] = 0.f;
}

template <int BMT>
static void launch_bf16w(const GemmArgs& a, int epi, hipStream_t s) {
  constexpr bool NARROW = BMT == 16;
  constexpr int BNT = NARROW ? 64 : 128;
  const int tiles = ((a.w.rows + BNT - 1) / BNT) * ((a.T + BMT - 1) / BMT);
  const int nk = a.w.K / W16_BK;
  // Split K until the grid fills the chip. Narrow: ~4 blocks (16 waves) per CU, >= 4 K steps (one
  // ring) per part - a 4096 x 4096 projection is 64 tiles x 16 parts. Wide: as gemm_dq, ~2 blocks
  // per CU and >= 8 steps per part.
  const int target = NARROW ? 1024 : 512, min_steps = NARROW ? 4 : 8;
  int split = 1;
  if (epi != GEMM_SWIGLU) {
    while (tiles * split < target && nk / (split * 2) >= min_steps) split *= 2;
  }
  if (split > 1 && epi == GEMM_STORE && !a.out_zeroed)
    hipLaunchKernelGGL(gemm_bf16w_zero_kernel, dim3(a.T), dim3(256), 0, s, a.out, a.ldo, a.w.rows);
  const dim3 grid((a.w.rows + BNT - 1) / BNT, (a.T + BMT - 1) / BMT, split), block(256);
  switch (epi) {
    case GEMM_STORE: hipLaunchKernelGGL((gemm_bf16w_kernel<GEMM_STORE, BMT>), grid, block, 0, s, a); break;
    case GEMM_ADD: hipLaunchKernelGGL((gemm_bf16w_kernel<GEMM_ADD, BMT>), grid, block, 0, s, a); break;
    case GEMM_SWIGLU: hipLaunchKernelGGL((gemm_bf16w_kernel<GEMM_SWIGLU, BMT>), grid, block, 0, s, a); break;
    default: throw std::runtime_error("gemm_bf16w: bad epilogue");
  }
}

void gemm_bf16w(const GemmArgs& a, int epi, hipStream_t s) {
  if (a.T <= 0) return;
  if (a.w.type != T_BF16) throw std::runtime_error("gemm_bf16w: BF16 weights only");
  if (a.w.K % W16_BK) throw std::runtime_error("gemm_bf16w: K must be a multiple of 64");
  if (a.seg_dev) throw std::runtime_error("gemm_bf16w: no grouped form (BF16 experts are not supported)");
  if (epi == GEMM_SWIGLU && (a.w.rows % 64)) throw std::runtime_error("gemm_bf16w: swiglu needs 64-row groups");
  if (a.T <= 16) launch_bf16w<16>(a, epi, s);
  else if (a.T <= 64) launch_bf16w<64>(a, epi, s);
  else launch_bf16w<128>(a, epi, s);
}

}  // namespace lfk
