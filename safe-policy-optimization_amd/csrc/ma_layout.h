// Multi-agent networks: the flat parameter / workspace layout and the kernels of the input LayerNorm's fold that the network
// passes (ma_net.hip) and the fused Fisher-vector product (ma_fvp.hip) share.
#pragma once
#include "common.h"
#include "../../include/safepo_hip.h"

namespace spo {

// ---------------------------------------------------------------- layout
struct Lay {
  int D, H, NB, O, actor;
  int64_t fn_g() const { return 0; }
  int64_t fn_b() const { return D; }
  int in_k(int k) const { return k == 0 ? D : H; }
  int64_t blk(int k) const {          // start of block k
    int64_t o = 2 * (int64_t)D;
    for (int i = 0; i < k; ++i) o += (int64_t)H * in_k(i) + 3 * (int64_t)H;
    return o;
  }
  int64_t W(int k) const { return blk(k); }
  int64_t b(int k) const { return blk(k) + (int64_t)H * in_k(k); }
  int64_t g(int k) const { return b(k) + H; }
  int64_t be(int k) const { return g(k) + H; }
  int64_t logstd() const { return blk(NB); }
  int64_t hW() const { return blk(NB) + (actor ? O : 0); }
  int64_t hb() const { return hW() + (int64_t)O * H; }
  int64_t count() const { return hb() + O; }
  // workspace (floats) for B rows: xhat[B,D], st0[B,2], per block: a[B,H], st[B,2], y[B,H]; every region starts on a
  // 16-byte boundary (row statistics padded to a multiple of 4 floats) so the 128-wide kernels can use float4 accesses
  static int64_t al4(int64_t n) { return (n + 3) & ~(int64_t)3; }
  int64_t ws_xhat() const { return 0; }
  int64_t ws_st0(int64_t B) const { return al4(B * D); }
  int64_t ws_blk(int64_t B, int k) const { return al4(B * D) + al4(2 * B) + (int64_t)k * (2 * al4(B * H) + al4(2 * B)); }
  int64_t ws_a(int64_t B, int k) const { return ws_blk(B, k); }
  int64_t ws_st(int64_t B, int k) const { return ws_blk(B, k) + al4(B * H); }
  int64_t ws_y(int64_t B, int k) const { return ws_blk(B, k) + al4(B * H) + al4(2 * B); }
  // block 0's weights with the input LayerNorm's affine folded in: W'[n][c] = W_0[n][c] * gamma[c], b'[n] = b_0[n] + W_0[n] . beta
  int64_t ws_w0f(int64_t B) const { return ws_blk(B, NB); }
  int64_t ws_b0f(int64_t B) const { return ws_w0f(B) + al4((int64_t)H * D); }
  int64_t ws_count(int64_t B) const { return ws_b0f(B) + al4(H); }
};

inline int lay_of(const spo_ma_net* n, Lay* L) {
  if (!n) return fail(-1, "ma: net is NULL");
  if (n->in_dim < 1 || n->in_dim > 512 || n->hidden < 1 || n->hidden > 512 || n->n_blocks < 1 || n->n_blocks > 8 ||
      n->out_dim < 1 || n->out_dim > 64)
    return fail(-2, "ma: net dims out of range (in %d, hidden %d, blocks %d, out %d; limits 512/512/8/64)", n->in_dim,
                n->hidden, n->n_blocks, n->out_dim);
  *L = Lay{n->in_dim, n->hidden, n->n_blocks, n->out_dim, n->is_actor ? 1 : 0};
  return 0;
}

__device__ __forceinline__ float wave_sum_all(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// W' = W_0 diag(gamma), b' = b_0 + W_0 beta  ->  their tangents (fold: ma_net.hip, fn_fold_kernel)
static __global__ void fn_fold_tangent_kernel(const float* __restrict__ W0, const float* __restrict__ gam, const float* __restrict__ bet,
                                       const float* __restrict__ tW0, const float* __restrict__ tb0, const float* __restrict__ tgam,
                                       const float* __restrict__ tbet, int H, int D, float* __restrict__ tWf, float* __restrict__ tbf) {
  const int n = blockIdx.x;                      // W' = W_0 diag(gamma), b' = b_0 + W_0 beta  ->  their tangents
  float dot = 0.f;
  for (int c = threadIdx.x; c < D; c += 64) {
    const float w = W0[(int64_t)n * D + c], tw = tW0[(int64_t)n * D + c];
    tWf[(int64_t)n * D + c] = tw * gam[c] + w * tgam[c];
    dot += tw * bet[c] + w * tbet[c];
  }
  dot = wave_sum_all(dot);
  if (threadIdx.x == 0) tbf[n] = tb0[n] + dot;
}
// grad + W(0) holds dW' = dz_0^T xn and db0 the column sums of dz_0 (fold: ma_net.hip, above fn_fold_kernel):
//   d(gamma)[c] = sum_n W_0[n][c] dW'[n][c],  d(beta)[c] = sum_n db_0[n] W_0[n][c],  dW_0[n][c] = gamma[c] dW'[n][c] + beta[c] db_0[n]
static __global__ void fn_unfold_grad_kernel(const float* __restrict__ W0, const float* __restrict__ gam, const float* __restrict__ bet,
                                      float* __restrict__ dW, const float* __restrict__ db0, int H, int D, float* __restrict__ dg,
                                      float* __restrict__ dbeta) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= D) return;
  const float gc = gam[c], bc = bet[c];
  float sg = 0.f, sb = 0.f;
  // 16 rows of loads in flight per step (one thread walks all H rows of its column: serial latency otherwise, 50 us at
  // H = 128); the sums keep their row order
  for (int n0 = 0; n0 < H; n0 += 16) {
    float w[16], dwp[16], dbn[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int n = n0 + u < H ? n0 + u : H - 1;
      w[u] = W0[(int64_t)n * D + c]; dwp[u] = dW[(int64_t)n * D + c]; dbn[u] = db0[n];
    }
#pragma unroll
    for (int u = 0; u < 16; ++u)
      if (n0 + u < H) {
        sg = fmaf(w[u], dwp[u], sg);
        sb = fmaf(dbn[u], w[u], sb);
        dW[(int64_t)(n0 + u) * D + c] = fmaf(gc, dwp[u], bc * dbn[u]);
      }
  }
  dg[c] = sg; dbeta[c] = sb;
}

}  // namespace spo
