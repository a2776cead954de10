// Plain fp32 MFMA GEMMs of the launch-per-layer paths: the multi-agent networks (ma_net.hip) and the wide single-agent
// networks (wide.hip).  Y = X W^T and dX = dY W on gemm_mfma_kernel (64 x 64 tiles), dW = dY^T X on the split-row pair
// dw_partial_kernel / dw_reduce_kernel.  Host functions: namespace spo, declared in gemm_f32.h.
#include <cstdlib>
#include "common.h"
#include "mlp_mfma.h"
#include "gemm_f32.h"
#include "../../include/safepo_hip.h"

namespace {

using spo::f4;

// ---------------------------------------------------------------- hand-written fp32 MFMA GEMM (all plain products)
// Y[B, N] (+)= X[B, R] * Wop[R, N], where the weight operand is addressed as Wop[r][j] = W[j * w_sj + r * w_sr]:
//   Y = X W^T  (forward blocks at small batch / hidden != 128, heads, tangent passes):  w_sj = R, w_sr = 1
//   dX = dY W  (head and non-fused block input gradients):                              w_sj = 1, w_sr = N_w (= K of W)
// 64 rows x 64 columns per workgroup, 4 waves x (16 rows x 64 columns), reduction in chunks of 32 staged through LDS
// (row stride 33: the 16 x 4 operand pattern of v_mfma_f32_16x16x4_f32 touches 32 different banks twice).  These shapes
// are launch-bound (8192 x 48..128 x 128 at collect time, heads with 1-16 columns), so the kernel is kept simple; the
// large-batch training products run in the fused block kernels of ma_net.hip and gemm128_kernel of wide.hip.
constexpr int GM_T = 64, GM_KC = 32, GM_LD = GM_KC + 1;
__global__ __launch_bounds__(256) void gemm_mfma_kernel(const float* __restrict__ X, const float* __restrict__ W, float* __restrict__ Y,
                                                        int64_t B, int R, int N, int64_t w_sj, int64_t w_sr, float beta) {
  __shared__ float Xs[GM_T * GM_LD];
  __shared__ float Ws[GM_T * GM_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, kq = lane >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * GM_T;          // rows on grid.x (2^31 - 1 tiles), the few column tiles on grid.y
  const int col0 = blockIdx.y * GM_T;
  f4 acc[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) acc[nt] = f4{0.f, 0.f, 0.f, 0.f};
  const int lr = tid >> 2, ls = (tid & 3) * 8;                  // staging: row / column lr, 8 reduction indices from ls
  for (int r0 = 0; r0 < R; r0 += GM_KC) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int r = r0 + ls + e;
      const int64_t xr = row0 + lr;
      Xs[lr * GM_LD + ls + e] = (xr < B && r < R) ? X[xr * R + r] : 0.f;
      const int wc = col0 + lr;
      Ws[lr * GM_LD + ls + e] = (wc < N && r < R) ? W[(int64_t)wc * w_sj + (int64_t)r * w_sr] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < GM_KC; kk += 4) {
      const float av = Xs[(16 * wave + i) * GM_LD + kk + kq];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
        acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, Ws[(16 * nt + i) * GM_LD + kk + kq], acc[nt], 0, 0, 0);
    }
    __syncthreads();
  }
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int64_t row = row0 + 16 * wave + 4 * kq + reg;
      const int col = col0 + 16 * nt + i;
      if (row < B && col < N) {
        float* const y = Y + row * N + col;
        *y = beta != 0.f ? fmaf(beta, *y, acc[nt][reg]) : acc[nt][reg];
      }
    }
}
// dW[N,K] = dY[B,N]^T * X[B,K]: a tiny output reduced over a huge row count.  rocBLAS runs this shape at 5 TFLOP/s
// (one 256x64 macro-tile marching over 524 288 rows: 3.15 ms at N = K = 128, 59 % of a MAPPO-L epoch); the shape is
// HBM-bound (both operands are read once: 537 MB -> ~0.15 ms), so it is done here: the rows are split over up to 256
// workgroups per 128x128 output tile, each accumulating its slice with fp32 MFMA from LDS-staged 32-row chunks, and a
// second kernel adds the slices in a fixed order.
#ifndef SPO_DW_R
#define SPO_DW_R 32
#endif
constexpr int DW_T = 128, DW_R = SPO_DW_R, DW_LD = DW_T + 16;      // row stride 144: the two row-groups of a half-wave land 16 banks apart

inline int64_t dw_max_splits() {            // SPO_DW_MAX_SPLITS: A/B knob (256 = the round-1/2 value)
  static const int64_t v = [] { const char* e = getenv("SPO_DW_MAX_SPLITS"); const int64_t x = e ? atoll(e) : 512; return x < 1 ? 1 : x; }();
  return v;
}

template <bool VEC>
__global__ __launch_bounds__(256, 2) void dw_partial_kernel(const float* __restrict__ dY, const float* __restrict__ X,
                                                            float* __restrict__ partial, int64_t B, int N, int K, int S) {
  __shared__ __attribute__((aligned(16))) float Ys[DW_R * DW_LD];
  __shared__ __attribute__((aligned(16))) float Xs[DW_R * DW_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, kk = lane >> 4;
  const int tiles_k = (K + DW_T - 1) / DW_T;
  const int tile = blockIdx.x / S, slice = blockIdx.x % S;
  const int n0 = (tile / tiles_k) * DW_T, k0 = (tile % tiles_k) * DW_T;
  const int64_t rows_per = ((B + S - 1) / S + DW_R - 1) / DW_R * DW_R;
  const int64_t r_begin = (int64_t)slice * rows_per;
  const int64_t r_end = r_begin + rows_per < B ? r_begin + rows_per : B;
  f4 acc[2][8];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int t = 0; t < 8; ++t) acc[m][t] = f4{0.f, 0.f, 0.f, 0.f};
  // The next 32-row chunk of both operands is fetched into registers while the current one is multiplied: with one or
  // two workgroups per CU nothing else hides the ~2 us load latency (318 -> ~190 us per call at 524 288 x 128 x 128).
  f4 py[DW_R / 8], px[DW_R / 8];
  auto fetch_chunk = [&](int64_t r0) {
#pragma unroll
    for (int q = 0; q < DW_R / 8; ++q) {
      const int idx = q * 256 + tid, row = idx >> 5, c4 = (idx & 31) * 4;
      const int64_t r = r0 + row;
      f4 y = {0.f, 0.f, 0.f, 0.f}, x = {0.f, 0.f, 0.f, 0.f};
      if (r < r_end) {
        if (VEC) {
          if (n0 + c4 < N) y = *reinterpret_cast<const f4*>(dY + r * N + n0 + c4);
          if (k0 + c4 < K) x = *reinterpret_cast<const f4*>(X + r * K + k0 + c4);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if (n0 + c4 + e < N) y[e] = dY[r * N + n0 + c4 + e];
            if (k0 + c4 + e < K) x[e] = X[r * K + k0 + c4 + e];
          }
        }
      }
      py[q] = y; px[q] = x;
    }
  };
  if (r_begin < r_end) fetch_chunk(r_begin);
  for (int64_t r0 = r_begin; r0 < r_end; r0 += DW_R) {
    // stage DW_R rows x 128 columns of both operands (zero beyond the matrix edges)
#pragma unroll
    for (int q = 0; q < DW_R / 8; ++q) {
      const int idx = q * 256 + tid, row = idx >> 5, c4 = (idx & 31) * 4;
      *reinterpret_cast<f4*>(Ys + row * DW_LD + c4) = py[q];
      *reinterpret_cast<f4*>(Xs + row * DW_LD + c4) = px[q];
    }
    __syncthreads();
    if (r0 + DW_R < r_end) fetch_chunk(r0 + DW_R);            // in flight during the MFMA loop
#pragma unroll
    for (int st = 0; st < DW_R / 4; ++st) {
      const float* yr = Ys + (4 * st + kk) * DW_LD + 32 * wave + i;
      const float* xr = Xs + (4 * st + kk) * DW_LD + i;
      const float a0 = yr[0], a1 = yr[16];
      float b[8];
#pragma unroll
      for (int t = 0; t < 8; ++t) b[t] = xr[16 * t];
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b[t], acc[0][t], 0, 0, 0);
        acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b[t], acc[1][t], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  // C layout: lane holds C[row = 4*(lane>>4) + e][col = lane & 15] of each 16x16 tile
  float* out = partial + (int64_t)slice * N * K;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int n = n0 + 32 * wave + 16 * m + 4 * kk + e, k = k0 + 16 * t + i;
        if (n < N && k < K) out[(int64_t)n * K + k] = acc[m][t][e];
      }
}
// 64 outputs x 16 strided groups of slices per workgroup (1024 threads), combined in a fixed order
__global__ __launch_bounds__(1024) void dw_reduce_kernel(const float* __restrict__ partial, int S, int64_t NK, float* __restrict__ out) {
  __shared__ float sh[16][64];
  const int c = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int64_t j = (int64_t)blockIdx.x * 64 + c;
  float s = 0.f;
  if (j < NK)
    for (int b = q; b < S; b += 16) s += partial[(int64_t)b * NK + j];
  sh[q][c] = s;
  __syncthreads();
  if (q == 0 && j < NK) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += sh[k][c];
    out[j] = t;
  }
}

}  // namespace

namespace spo {

int gemm_mfma(hipStream_t st, const float* X, const float* W, float* Y, int64_t B, int R, int N, int64_t w_sj, int64_t w_sr,
              float beta) {
  const int64_t row_tiles = (B + GM_T - 1) / GM_T, col_tiles = (N + GM_T - 1) / GM_T;
  if (row_tiles > 0x7fffffffLL || col_tiles > 65535)
    return spo::fail(-1, "ma gemm: %lld x %d exceeds the launch grid (row tiles %lld, column tiles %lld)", (long long)B, N,
                     (long long)row_tiles, (long long)col_tiles);
  const dim3 grid((unsigned)row_tiles, (unsigned)col_tiles);
  hipLaunchKernelGGL(gemm_mfma_kernel, grid, dim3(256), 0, st, X, W, Y, B, R, N, w_sj, w_sr, beta);
  return 0;
}
// Row-major helpers.  Y[B,N] (+)= X[B,K] * W[N,K]^T
int gemm_xwT(hipStream_t st, const float* X, const float* W, float* Y, int64_t B, int K, int N, float beta) {
  return gemm_mfma(st, X, W, Y, B, K, N, K, 1, beta);
}
// dX[B,K] = dY[B,N] * W[N,K]
int gemm_dyw(hipStream_t st, const float* dY, const float* W, float* dX, int64_t B, int K, int N) {
  return gemm_mfma(st, dY, W, dX, B, N, K, 1, K, 0.f);
}
int dw_splits(int64_t B, int N, int K) {
  const int64_t tiles = (int64_t)((N + DW_T - 1) / DW_T) * ((K + DW_T - 1) / DW_T);
  int64_t s = (B + 255) / 256;                       // at least 256 rows per slice
  const int64_t cap_mem = (int64_t)(1 << 24) / ((int64_t)N * K) > 0 ? (int64_t)(1 << 24) / ((int64_t)N * K) : 1;   // <= 64 MB of slices
  const int64_t cap_grid = 2048 / tiles > 0 ? 2048 / tiles : 1;
  // two (three) workgroups per CU: 256 slices were ONE workgroup per CU -- one wave per SIMD, every barrier and load exposed
  if (s > dw_max_splits()) s = dw_max_splits();
  if (s > cap_mem) s = cap_mem;
  if (s > cap_grid) s = cap_grid;
  return (int)(s < 1 ? 1 : s);
}
// `slices`: float[dw_splits(B, N, K) * N * K]
int gemm_dyTx(hipStream_t st, const float* dY, const float* X, float* dW, int64_t B, int K, int N, float* slices) {
  const int S = dw_splits(B, N, K);
  const int tiles = ((N + DW_T - 1) / DW_T) * ((K + DW_T - 1) / DW_T);
  const bool vec = (N % 4 == 0) && (K % 4 == 0) && ((reinterpret_cast<uintptr_t>(dY) | reinterpret_cast<uintptr_t>(X)) % 16 == 0);
  if (vec) hipLaunchKernelGGL(dw_partial_kernel<true>, dim3(tiles * S), dim3(256), 0, st, dY, X, slices, B, N, K, S);
  else hipLaunchKernelGGL(dw_partial_kernel<false>, dim3(tiles * S), dim3(256), 0, st, dY, X, slices, B, N, K, S);
  const int64_t NK = (int64_t)N * K;
  hipLaunchKernelGGL(dw_reduce_kernel, dim3((unsigned)((NK + 63) / 64)), dim3(1024), 0, st, slices, S, NK, dW);
  return 0;
}

}  // namespace spo

// Test comparator: Y[B,N] = X[B,K] W[N,K]^T (mode 0) or dX[B,K] = dY[B,N] W[N,K] (mode 1) through the hand-written MFMA
// kernel.  use_rocblas must be 0: the rocBLAS comparator was removed (tests compare with torch.matmul instead).
extern "C" int spo_debug_ma_gemm(int use_rocblas, int mode, const float* x, const float* w, float* y, int64_t B, int K, int N,
                                 void* stream) {
  SPO_REQUIRE(x && w && y && B > 0 && K > 0 && N > 0 && (mode == 0 || mode == 1), "debug_ma_gemm: bad args");
  SPO_REQUIRE(!use_rocblas, "debug_ma_gemm: the rocBLAS comparator was removed; use_rocblas must be 0");
  if (int rc = mode == 0 ? spo::gemm_xwT((hipStream_t)stream, x, w, y, B, K, N) : spo::gemm_dyw((hipStream_t)stream, x, w, y, B, K, N))
    return rc;
  SPO_LAUNCH_CHECK("spo_debug_ma_gemm");
  return 0;
}
