// Plain fp32 MFMA GEMMs shared by the multi-agent networks (ma_net.hip) and the wide single-agent path (wide.hip);
// defined in gemm_f32.hip.  Row-major operands, launches on `st`, 0 or a negative error code.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace spo {

// Y[B, N] (+)= X[B, R] * Wop[R, N] with Wop[r][j] = W[j * w_sj + r * w_sr]; beta != 0: Y = beta * Y + product
int gemm_mfma(hipStream_t st, const float* X, const float* W, float* Y, int64_t B, int R, int N, int64_t w_sj, int64_t w_sr, float beta);
// Y[B,N] (+)= X[B,K] * W[N,K]^T
int gemm_xwT(hipStream_t st, const float* X, const float* W, float* Y, int64_t B, int K, int N, float beta = 0.f);
// dX[B,K] = dY[B,N] * W[N,K]
int gemm_dyw(hipStream_t st, const float* dY, const float* W, float* dX, int64_t B, int K, int N);
// dW[N,K] = dY[B,N]^T * X[B,K] through `slices`: float[dw_splits(B, N, K) * N * K]
int dw_splits(int64_t B, int N, int K);
int gemm_dyTx(hipStream_t st, const float* dY, const float* X, float* dW, int64_t B, int K, int N, float* slices);

}  // namespace spo
