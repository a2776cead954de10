// Wide single-agent networks: ActorVCritic(obs_dim, act_dim, hidden_sizes) for ANY hidden_sizes (reference
// safepo/common/model.py:30-48,131; isaac_gym_specific_cfg uses [1024, 1024, 512] with minibatches of 8 192 rows,
// safepo/single_agent/ppo_lag.py:54-65).  The persistent kernels of update.hip keep a 64-wide network in one CU's LDS for
// thousands of dependent 64-row steps; a wide network at a wide batch is the opposite regime -- a handful of large steps
// per epoch, each a chain of real GEMMs -- so it runs as a sequence of launches on the in-tree fp32 MFMA GEMM kernels
// (gemm_f32.hip: X W^T, dY W, dY^T X; gemm128_kernel below) with small elementwise kernels between them:
//   forward   h_l = tanh(h_{l-1} W_l^T + b_l), last layer linear                      spo_mlp_forward
//   backward  dZ_l = dH_l (1 - h_l^2); db_l = colsum dZ_l; dW_l = dZ_l^T h_{l-1}; dH_{l-1} = dZ_l W_l     spo_mlp_backward
//   losses    MSE critics, clipped PPO surrogate + d(log_std) (ppo_lag.py:306-323)     spo_wide_ppo_loss
//   step      critic L2 terms, joint clip_grad_norm_, Adam (ppo_lag.py:310-329)        spo_wide_clip_adam
// Flat parameter layout of one network: for every Linear in order, W [out, in] row-major then b [out] -- the order of
// nn.Sequential.parameters(), so the module's parameters stay views of one vector (log_std precedes the actor's layers).
//
// This is also the fallback for ANY (obs_dim, act_dim, hidden_sizes) and for every single-agent script (reference model.py:131
// takes any dims; benchmark.py:5-22 pairs cpo / pcpo / rcpo / trpo_lag / focops / cup with Car, Doggo, Racecar (obs 72-88) and
// HumanoidVelocity (obs 376, act 17)).  The LDS-resident kernels keep their envelope (obs <= 128, act <= 16; CPO full-batch
// kernels obs <= 64); everything outside it runs here:
//   spo_wide_actor_loss       clipped surrogate | plain surrogate sign*mean(ratio*adv) | KL-penalty (FOCOPS, CUP stage 2)
//   spo_wide_critic_loss      MSE of both critics + output gradients (critic fit, cpo.py:541-571)
//   spo_mlp_jvp               forward-mode tangent d(out)/d(theta).t of the tanh MLP (Fisher-vector product, cpo.py:132-157)
//   spo_wide_fvp_cotangent    (J t) / sigma^2 / (rows_total * act_dim)
//   spo_wide_linesearch_sums  sum ratio*adv_a, sum ratio*adv_b, sum KL(old || new)   (cpo.py:473-491)
//   spo_wide_clip_adam_ex     joint clip over all parameters, Adam on a sub-range with per-optimiser step counts, stale
//                             gradients outside the range rescaled in place (what clip_grad_norm_ does to actor.grad in the
//                             critic fit, cpo.py:557; CUP's actor-only second stage, cup.py:385)
//   spo_wide_clip_adam_dev    the same with the optimiser clocks on the device, so a step can be captured and replayed
// Layout of this file: kernels and host helpers first (one anonymous namespace), then the C entry points.
#include <cmath>
#include "common.h"
#include "adam.h"
#include "adam_host.h"
#include "mlp_mfma.h"
#include "mlp_small.h"
#include "gemm_f32.h"
#include "wide_opt.h"
#include "../../include/safepo_hip.h"

namespace {
using namespace spo;

// ---- 128 x 128-tile fp32 MFMA GEMM for the wide networks (round 3).  gemm_mfma_kernel of gemm_f32.hip (64 x 64 tiles, scalar staging)
// serves launch-bound shapes; a [1024, 1024, 512] network at 8 192 rows is a chain of real GEMMs (17 GFLOP each), so:
//   TRANSB = false:  Y[B, N] = act(X[B, K] W[N, K]^T + bias)            (forward: both operands K-contiguous)
//   TRANSB = true :  Y[B, N] = (X[B, K] W[K, N]) * (1 - Hm[B, N]^2)      (input gradient dY W with the tanh' factor fused)
// One workgroup = 128 x 128 outputs, 2 x 2 waves of 64 x 64 (16 accumulator tiles per wave); the reduction runs in chunks of
// 16 staged through LDS with row stride 20 floats -- a lane's ds_read_b128 at [row][4q] is the operand of four consecutive
// MFMA steps (k = 4q + r, the enumeration of mlp_mfma.h), and 20 i mod 64 walks all sixteen 4-bank groups, so the sixteen
// lanes of a read phase never collide.  The next chunk is fetched into registers while the current one is multiplied.
// Requirements (else the caller falls back to gemm_mfma_kernel): K % 4 == 0 (TRANSB: N % 4 == 0), 16-byte aligned operands.
constexpr int G2_T = 128, G2_K = 16, G2_LD = 20;
template <bool TRANSB>
__global__ __launch_bounds__(256) void gemm128_kernel(const float* __restrict__ X, const float* __restrict__ W, float* __restrict__ Y,
                                                      int64_t B, int K, int N, const float* __restrict__ bias, int tanh_on,
                                                      const float* __restrict__ Hm, int w_vec) {
  __shared__ __attribute__((aligned(16))) float As[G2_T * G2_LD];
  __shared__ __attribute__((aligned(16))) float Bs[G2_T * G2_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, q = lane >> 4;
  const int wr = wave >> 1, wc = wave & 1;
  const int64_t row0 = (int64_t)blockIdx.x * G2_T;
  const int col0 = blockIdx.y * G2_T;
  f4 acc[4][4];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = f4{0.f, 0.f, 0.f, 0.f};
  // staging assignment.  A (and B when it is K-contiguous): thread -> row tid / 2, eight k from (tid & 1) * 8.
  // TRANSB B: thread -> reduction row tid / 16 of the chunk, eight output columns from (tid & 15) * 8 (stored transposed).
  const int sa_r = tid >> 1, sa_k = (tid & 1) * 8;
  const int sb_n = tid >> 4, sb_c = (tid & 15) * 8;
  f4 pa[2], pb[2];
  auto fetch = [&](int k0) {
    const int64_t r = row0 + sa_r;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = k0 + sa_k + 4 * h;
      pa[h] = (r < B && k < K) ? *reinterpret_cast<const f4*>(X + r * K + k) : f4{0.f, 0.f, 0.f, 0.f};
    }
    if (!TRANSB) {
      const int c = col0 + sa_r;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int k = k0 + sa_k + 4 * h;
        pb[h] = f4{0.f, 0.f, 0.f, 0.f};
        if (c < N && k < K) {
          const float* src = W + (int64_t)c * K + k;            // a network's slice of the flat vector need not be 16-byte aligned
          if (w_vec) pb[h] = *reinterpret_cast<const f4*>(src);
          else pb[h] = f4{src[0], src[1], src[2], src[3]};
        }
      }
    } else {
      const int k = k0 + sb_n;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int c = col0 + sb_c + 4 * h;
        pb[h] = f4{0.f, 0.f, 0.f, 0.f};
        if (k < K && c < N) {
          const float* src = W + (int64_t)k * N + c;
          if (w_vec) pb[h] = *reinterpret_cast<const f4*>(src);
          else pb[h] = f4{src[0], src[1], src[2], src[3]};
        }
      }
    }
  };
  fetch(0);
  for (int k0 = 0; k0 < K; k0 += G2_K) {
#pragma unroll
    for (int h = 0; h < 2; ++h) *reinterpret_cast<f4*>(As + sa_r * G2_LD + sa_k + 4 * h) = pa[h];
    if (!TRANSB) {
#pragma unroll
      for (int h = 0; h < 2; ++h) *reinterpret_cast<f4*>(Bs + sa_r * G2_LD + sa_k + 4 * h) = pb[h];
    } else {
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int e = 0; e < 4; ++e) Bs[(sb_c + 4 * h + e) * G2_LD + sb_n] = pb[h][e];
    }
    __syncthreads();
    if (k0 + G2_K < K) fetch(k0 + G2_K);                       // in flight during the 64 MFMAs below
    f4 a[4], b[4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) a[rt] = *reinterpret_cast<const f4*>(As + (64 * wr + 16 * rt + i) * G2_LD + 4 * q);
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) b[ct] = *reinterpret_cast<const f4*>(Bs + (64 * wc + 16 * ct + i) * G2_LD + 4 * q);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
          acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rt][r], b[ct][r], acc[rt][ct], 0, 0, 0);
    __syncthreads();
  }
  // C layout: lane holds rows 4q + e, column i of every 16 x 16 tile
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const int col = col0 + 64 * wc + 16 * ct + i;
      if (col >= N) continue;
      const float bv = bias ? bias[col] : 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t row = row0 + 64 * wr + 16 * rt + 4 * q + e;
        if (row >= B) continue;
        float v = acc[rt][ct][e] + bv;
        if (tanh_on) v = fast_tanh(v);
        if (Hm) { const float hv = Hm[row * N + col]; v = v * fmaf(-hv, hv, 1.f); }
        Y[row * N + col] = v;
      }
    }
}
// true when the 128-tile kernel applies (big enough to fill tiles, aligned, vectorisable)
inline bool gemm128_ok(const float* X, int64_t B, int K, int N, bool transb) {
  if (B < 256 || N < 64 || K < 16) return false;
  if (((B + G2_T - 1) / G2_T) * ((N + G2_T - 1) / G2_T) < 192) return false;      // too few 128 x 128 tiles to fill 256 CUs
  if (reinterpret_cast<uintptr_t>(X) & 15) return false;
  return transb ? (K % 4 == 0 && N % 4 == 0) : (K % 4 == 0);
}
inline int w_is_vec(const float* W) { return (reinterpret_cast<uintptr_t>(W) & 15) == 0 ? 1 : 0; }

// ---- the tanh MLP: layout of a network in the flat vector, elementwise kernels between the GEMMs
struct MlpLay {
  int n;                 // Linear layers
  int d[SPO_MLP_MAX_LAYERS + 1];
  int64_t w(int l) const { int64_t o = 0; for (int k = 0; k < l; ++k) o += (int64_t)d[k + 1] * d[k] + d[k + 1]; return o; }
  int64_t b(int l) const { return w(l) + (int64_t)d[l + 1] * d[l]; }
  int64_t count() const { return w(n); }
  int64_t act_off(int l, int64_t rows) const { int64_t o = 0; for (int k = 0; k < l; ++k) o += rows * d[k + 1]; return o; }   // h_{l+1} inside ws
  int maxdim() const { int m = 0; for (int k = 0; k <= n; ++k) m = d[k] > m ? d[k] : m; return m; }
};
int mlp_lay(const spo_mlp_net* net, MlpLay* L) {
  if (!net) return fail(-1, "mlp: net is NULL");
  if (net->n_layers < 1 || net->n_layers > SPO_MLP_MAX_LAYERS) return fail(-2, "mlp: n_layers %d outside [1,%d]", net->n_layers, SPO_MLP_MAX_LAYERS);
  L->n = net->n_layers;
  for (int k = 0; k <= L->n; ++k) {
    if (net->dims[k] < 1 || net->dims[k] > 16384) return fail(-2, "mlp: dims[%d] = %d outside [1,16384]", k, net->dims[k]);
    L->d[k] = net->dims[k];
  }
  return 0;
}

__global__ __launch_bounds__(256) void mlp_bias_act_kernel(float* __restrict__ y, const float* __restrict__ b, int64_t n, int N, int tanh_on) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float v = y[i] + b[i % N];
    y[i] = tanh_on ? fast_tanh(v) : v;
  }
}
__global__ __launch_bounds__(256) void mlp_dtanh_kernel(float* __restrict__ dh, const float* __restrict__ h, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float hv = h[i];
    dh[i] = dh[i] * fmaf(-hv, hv, 1.f);
  }
}
// column sums in two fixed-order stages: partial[s][c] over row slice s, then over the slices
constexpr int CS_SLICES = 64;
__global__ __launch_bounds__(256) void mlp_colsum_partial_kernel(const float* __restrict__ d, int64_t B, int N, float* __restrict__ partial) {
  const int c = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
  if (c >= N) return;
  const int64_t per = (B + CS_SLICES - 1) / CS_SLICES, r0 = s * per, r1 = r0 + per < B ? r0 + per : B;
  float acc = 0.f;
  int64_t r = r0;
  for (; r + 8 <= r1; r += 8) {                       // eight loads in flight, added in row order
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = d[(r + u) * N + c];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += v[u];
  }
  for (; r < r1; ++r) acc += d[r * N + c];
  partial[(int64_t)s * N + c] = acc;
}
__global__ __launch_bounds__(256) void mlp_colsum_finish_kernel(const float* __restrict__ partial, int N, float* __restrict__ out) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= N) return;
  float acc = 0.f;
  for (int s = 0; s < CS_SLICES; ++s) acc += partial[(int64_t)s * N + c];
  out[c] = acc;
}
int ew_grid(int64_t n) { const int64_t g = (n + 255) / 256; return (int)(g > 4096 ? 4096 : (g < 1 ? 1 : g)); }
// tangent epilogue of one layer: y = (y + tb) * (1 - h^2)  (hidden layers) or y + tb (output layer)
__global__ __launch_bounds__(256) void mlp_jvp_ew_kernel(float* __restrict__ y, const float* __restrict__ tb, const float* __restrict__ h,
                                                         int64_t n, int N) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    float v = y[i] + tb[i % N];
    if (h) { const float hv = h[i]; v = v * fmaf(-hv, hv, 1.f); }
    y[i] = v;
  }
}

// ---- Gaussian head: sample, KL
// a = mean + exp(log_std) * eps (rsample), logp = Normal(mean, exp(log_std)).log_prob(a).sum(-1)   (model.py:149-170)
__global__ __launch_bounds__(256) void gauss_sample_kernel(const float* __restrict__ mean, const float* __restrict__ log_std,
                                                           const float* __restrict__ eps, float* __restrict__ act, float* __restrict__ logp,
                                                           int64_t B, int A) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= B) return;
  float lp = 0.f;
  for (int k = 0; k < A; ++k) {
    const float sd = expf(log_std[k]), mu = mean[r * A + k];
    const float ac = eps ? mu + eps[r * A + k] * sd : mu;
    const float diff = ac - mu, var = sd * sd;
    lp += -(diff * diff) / (2.f * var) - logf(sd) - LOG_SQRT_2PI;
    act[r * A + k] = ac;
  }
  logp[r] = lp;
}
// sum over rows of KL(N(mean_old, std_old) || N(mean_new, std_new)).sum(-1)   (torch kl_normal_normal, ppo_lag.py:338-345)
__global__ __launch_bounds__(256) void gauss_kl_kernel(const float* __restrict__ mean_old, const float* __restrict__ log_std_old,
                                                       const float* __restrict__ mean_new, const float* __restrict__ log_std_new, int64_t B,
                                                       int A, double* __restrict__ partial) {
  __shared__ double red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double acc = 0.0;
  for (int64_t r = (int64_t)blockIdx.x * 256 + tid; r < B; r += (int64_t)gridDim.x * 256) {
    float kl = 0.f;
    for (int k = 0; k < A; ++k) {
      const float so = expf(log_std_old[k]), sn = expf(log_std_new[k]);
      const float ratio = so / sn, var_ratio = ratio * ratio;
      const float dm = (mean_old[r * A + k] - mean_new[r * A + k]) / sn;
      kl += 0.5f * (var_ratio + dm * dm - 1.f - logf(var_ratio));
    }
    acc += (double)kl;
  }
  acc = wave_sum_d(acc);
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (tid == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ void gauss_kl_finish_kernel(const double* __restrict__ partial, int nblocks, double* __restrict__ sum_inout, int accumulate) {
  if (threadIdx.x != 0) return;
  double s = accumulate ? sum_inout[0] : 0.0;
  for (int b = 0; b < nblocks; ++b) s += partial[b];
  sum_inout[0] = s;
}

// Rows idx[0 .. n) of up to SPO_GATHER_MAX row-major arrays (widths[k] floats per row) in one launch: the minibatch gather of a
// step (ppo_lag.py:298-305: the DataLoader's index_select of obs, act, log_prob, targets, advantage) instead of one launch per array.
struct GatherArgs {
  const float* src[SPO_GATHER_MAX];
  float* dst[SPO_GATHER_MAX];
  int width[SPO_GATHER_MAX];
  int count;
  const int64_t* idx;
  const int64_t* cursor;       // optional (device): the window idx[*cursor .. *cursor + n) -- a captured launch then walks a permutation
  int64_t n;
};
__global__ __launch_bounds__(256) void gather_rows_kernel(GatherArgs a) {
  const int k = blockIdx.y;
  const int w = a.width[k];
  const float* __restrict__ src = a.src[k];
  float* __restrict__ dst = a.dst[k];
  const int64_t* __restrict__ idx = a.idx + (a.cursor ? a.cursor[0] : 0);
  const int64_t total = a.n * w;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t r = e / w;
    const int c = (int)(e - r * w);
    dst[e] = src[idx[r] * w + c];
  }
}

// ---- losses
// PPO-Lagrangian losses and output gradients of one minibatch (ppo_lag.py:306-323): one thread per row.
constexpr int WL_NS = 3 + SPO_MAX_ACT;       // loss_r sum, loss_c sum, surrogate sum, d(log_std)[A]
__global__ __launch_bounds__(256) void wide_ppo_loss_kernel(const float* __restrict__ v_r, const float* __restrict__ v_c, const float* __restrict__ mean,
                                                            const float* __restrict__ log_std, const float* __restrict__ act,
                                                            const float* __restrict__ logp_old, const float* __restrict__ adv,
                                                            const float* __restrict__ tgt_r, const float* __restrict__ tgt_c, int64_t B, int A,
                                                            float clip, float* __restrict__ d_vr, float* __restrict__ d_vc,
                                                            float* __restrict__ d_mean, double* __restrict__ partial,
                                                            float* __restrict__ losses3, float* __restrict__ d_log_std) {
  // losses3 / d_log_std: given for a one-workgroup launch (minibatch-sized row counts), which finishes the sums itself -- the
  // same values wide_ppo_loss_finish_kernel forms from one partial row, one launch less
  __shared__ double red[4][WL_NS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float inv_n = 1.f / (float)B, clip_lo = 1.f - clip, clip_hi = 1.f + clip;
  double acc[WL_NS];
#pragma unroll
  for (int k = 0; k < WL_NS; ++k) acc[k] = 0.0;
  for (int64_t r = (int64_t)blockIdx.x * 256 + tid; r < B; r += (int64_t)gridDim.x * 256) {
    const float dr = v_r[r] - tgt_r[r], dc = v_c[r] - tgt_c[r];
    acc[0] += (double)(dr * dr); acc[1] += (double)(dc * dc);
    d_vr[r] = 2.f * dr * inv_n; d_vc[r] = 2.f * dc * inv_n;
    float lp = 0.f, dif[SPO_MAX_ACT], ivar[SPO_MAX_ACT];
    for (int k = 0; k < A; ++k) {
      const float ls = log_std[k], sd = __expf(ls);
      ivar[k] = 1.f / (sd * sd);
      dif[k] = act[r * A + k] - mean[r * A + k];
      lp += -(dif[k] * dif[k]) * (0.5f * ivar[k]) - ls - LOG_SQRT_2PI;
    }
    const float ad = adv[r];
    const float ratio = __expf(lp - logp_old[r]);
    const float rc = fminf(fmaxf(ratio, clip_lo), clip_hi);
    const float s1 = ratio * ad, s2 = rc * ad;
    const bool inr = (ratio >= clip_lo) && (ratio <= clip_hi);
    float gr;                                          // backward of torch.min / torch.clamp (ties split the gradient)
    if (s1 < s2) gr = ad;
    else if (s1 > s2) gr = inr ? ad : 0.f;
    else gr = 0.5f * ad + (inr ? 0.5f * ad : 0.f);
    const float dlp = -(gr * ratio) * inv_n;
    acc[2] += (double)fminf(s1, s2);
    for (int k = 0; k < A; ++k) {
      const float z = dif[k] * ivar[k];
      d_mean[r * A + k] = dlp * z;
      acc[3 + k] += (double)(dlp * (dif[k] * z - 1.f));
    }
  }
  for (int k = 0; k < 3 + A; ++k) {
    const double v = wave_sum_d(acc[k]);
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (tid < 3 + A) {
    const double v = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
    partial[(int64_t)blockIdx.x * WL_NS + tid] = v;
    if (losses3) {
      const double s = 0.0 + v;
      if (tid < 2) losses3[tid] = (float)(s / (double)B);
      else if (tid == 2) losses3[2] = (float)(-s / (double)B);
      else d_log_std[tid - 3] = (float)s;
    }
  }
}
__global__ void wide_ppo_loss_finish_kernel(const double* __restrict__ partial, int nblocks, int A, int64_t B, float* __restrict__ losses3,
                                            float* __restrict__ d_log_std) {
  const int k = threadIdx.x;
  if (k >= 3 + A) return;
  double s = 0.0;
  for (int b = 0; b < nblocks; ++b) s += partial[(int64_t)b * WL_NS + k];
  if (k < 2) losses3[k] = (float)(s / (double)B);
  else if (k == 2) losses3[2] = (float)(-s / (double)B);
  else d_log_std[k - 3] = (float)s;
}

// Actor-side loss kernels use G = pow2ceil(act_dim) lanes per row (act_dim <= SPO_WIDE_MAX_ACT = 64): coalesced loads along the
// action dimension, segmented xor-shuffle sums, no per-thread arrays.
constexpr int WA_NS = 2 + SPO_WIDE_MAX_ACT;      // partial row of an actor-loss block: loss sum, aux sum, d(log_std)[A]
enum { WA_CLIP = 0, WA_SURR = 1, WA_KLPEN = 2, WA_KLPEN_COUNT = 3 };

__device__ __forceinline__ float group_sum_f(float v, int G) {
  for (int o = 1; o < G; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// sum of a double over the lanes of the wave that hold the same action index (lanes k, k + G, k + 2G, ...)
__device__ __forceinline__ double stride_sum_d(double v, int G) {
  for (int o = G; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}
inline int pow2ceil(int a) { int g = 1; while (g < a) g <<= 1; return g; }

struct WaArgs {
  const float* mean; const float* log_std; const float* act; const float* logp_old; const float* adv;
  const float* old_mean; const float* old_std;
  int64_t B; int A, G;
  float p0, p1;                 // WA_CLIP: clip, -   WA_SURR: sign, -   WA_KLPEN: kl_bound, pg_coef
  float inv_n;                  // 1 / rows the mean is taken over
  const double* frac_sum;       // WA_KLPEN: device sum of the indicators (from the WA_KLPEN_COUNT pass), mean = frac_sum * inv_n
  float* d_mean; double* partial;
};

template <int MODE>
__global__ __launch_bounds__(256) void wide_actor_loss_kernel(WaArgs a) {
  __shared__ double red[4][WA_NS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int A = a.A, G = a.G, k = lane & (G - 1), sub = lane / G, rpw = 64 / G;
  const bool on = k < A;
  const float ls = on ? a.log_std[k] : 0.f;
  const float sd = __expf(ls), ivar = 1.f / (sd * sd);
  float iso = 1.f, vrat = 1.f, lvrat = 0.f;
  if (MODE == WA_KLPEN || MODE == WA_KLPEN_COUNT) {
    iso = on ? 1.f / a.old_std[k] : 1.f;
    const float sr = sd * iso;                      // kl_normal_normal: var_ratio = (p.scale / q.scale)^2
    vrat = sr * sr; lvrat = logf(vrat);
  }
  const float clip_lo = 1.f - a.p0, clip_hi = 1.f + a.p0;
  float frac = 0.f;
  if (MODE == WA_KLPEN) frac = (float)a.frac_sum[0] * a.inv_n;
  double s_loss = 0.0, s_aux = 0.0, s_dls = 0.0;
  const int64_t wave_g = (int64_t)blockIdx.x * 4 + wave, nwaves = (int64_t)gridDim.x * 4;
  for (int64_t r0 = wave_g * rpw; r0 < a.B; r0 += nwaves * rpw) {
    const int64_t r = r0 + sub;
    const bool rv = r < a.B;
    const int64_t rr = rv ? r : a.B - 1;
    const bool ld = on;
    const float mu = ld ? a.mean[rr * A + k] : 0.f;
    const float ac = ld ? a.act[rr * A + k] : 0.f;
    const float dif = ac - mu;
    const float term = on ? -(dif * dif) * (0.5f * ivar) - ls - LOG_SQRT_2PI : 0.f;
    const float lp = group_sum_f(term, G);
    float kl = 0.f, dm = 0.f;
    if (MODE == WA_KLPEN || MODE == WA_KLPEN_COUNT) {
      dm = on ? (mu - a.old_mean[rr * A + k]) * iso : 0.f;          // (loc_p - loc_q) / scale_q
      kl = group_sum_f(on ? 0.5f * (vrat + dm * dm - 1.f - lvrat) : 0.f, G);
    }
    if (MODE == WA_KLPEN_COUNT) {
      if (rv && k == 0) s_aux += (kl <= a.p0) ? 1.0 : 0.0;
      continue;
    }
    const float ad = a.adv[rr];
    const float ratio = __expf(lp - a.logp_old[rr]);
    float dlp, wk = 0.f;
    if (MODE == WA_CLIP) {
      const float rc = fminf(fmaxf(ratio, clip_lo), clip_hi);
      const float s1 = ratio * ad, s2 = rc * ad;
      const bool inr = (ratio >= clip_lo) && (ratio <= clip_hi);
      float gr;                                        // backward of torch.min / torch.clamp (ties split the gradient)
      if (s1 < s2) gr = ad;
      else if (s1 > s2) gr = inr ? ad : 0.f;
      else gr = 0.5f * ad + (inr ? 0.5f * ad : 0.f);
      dlp = -(gr * ratio) * a.inv_n;
      if (rv && k == 0) s_loss += (double)fminf(s1, s2);
    } else if (MODE == WA_SURR) {
      dlp = a.p0 * ad * ratio * a.inv_n;               // d(sign * mean(ratio * adv)) / d logp
      if (rv && k == 0) s_loss += (double)(ratio * ad);
    } else {
      const float ind = (kl <= a.p0) ? 1.f : 0.f;
      const float pg = a.p1 * frac;
      dlp = -(pg * ad * ratio) * a.inv_n;
      wk = ind * a.inv_n;
      if (rv && k == 0) { s_loss += (double)(pg * ratio * ad - ind * kl); s_aux += (double)ind; }      // loss = -mean(this)
    }
    if (rv && on) {
      const float z = dif * ivar;
      float dmu = dlp * z, dl = dlp * (dif * z - 1.f);
      if (MODE == WA_KLPEN) { dmu = fmaf(dlp, z, wk * dm * iso); dl = fmaf(dlp, dif * z - 1.f, wk * (vrat - 1.f)); }
      a.d_mean[r * A + k] = dmu;
      s_dls += (double)dl;
    }
  }
  s_loss = wave_sum_d(s_loss); s_aux = wave_sum_d(s_aux);
  s_dls = stride_sum_d(s_dls, G);
  if (lane == 0) { red[wave][0] = s_loss; red[wave][1] = s_aux; }
  if (lane < G && lane < A) red[wave][2 + lane] = s_dls;
  __syncthreads();
  if (tid < 2 + A) a.partial[(int64_t)blockIdx.x * WA_NS + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}
// sums[0] = loss sum, sums[1] = aux sum, sums[2 + k] = d(log_std)[k]; optional float outputs for the unchunked minibatch use
__global__ void wide_actor_loss_finish_kernel(const double* __restrict__ partial, int nblocks, int A, double* __restrict__ sums,
                                              int accumulate, float loss_scale, float* __restrict__ loss_out,
                                              float* __restrict__ d_log_std_out) {
  const int k = threadIdx.x;
  if (k >= 2 + A) return;
  double s = accumulate ? sums[k] : 0.0;
  for (int b = 0; b < nblocks; ++b) s += partial[(int64_t)b * WA_NS + k];
  sums[k] = s;
  if (k == 0 && loss_out) loss_out[0] = (float)(s * (double)loss_scale);
  if (k >= 2 && d_log_std_out) d_log_std_out[k - 2] = (float)s;
}

// Split KL-penalty form (data-parallel FOCOPS / CUP on the wide path, spo_wide_kl_penalty_split): the fraction F = mean_i(ind_i)
// belongs to the GLOBAL minibatch, and the gradient is linear in it, g = g_KL + F g_PG.  One pass emits both cotangents --
// d_mean_kl = ind_i d(KL_i)/d(mean) / n, d_mean_pg = -(pg_coef / n) d(ratio_i adv_i)/d(mean) (F taken as 1) -- the two parts of
// d(log_std), and the row sums (count of ind, sum ind*KL, sum ratio*adv); the caller all-reduces and combines with the global F.
constexpr int WAS_NS = 3 + 2 * SPO_WIDE_MAX_ACT;   // partial row: sum ind*KL, count, sum ratio*adv, d(log_std) KL[A], PG[A]
__global__ __launch_bounds__(256) void wide_klpen_split_kernel(WaArgs a, float* __restrict__ d_mean_pg) {
  __shared__ double red[4][WAS_NS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int A = a.A, G = a.G, k = lane & (G - 1), sub = lane / G, rpw = 64 / G;
  const bool on = k < A;
  const float ls = on ? a.log_std[k] : 0.f;
  const float sd = __expf(ls), ivar = 1.f / (sd * sd);
  const float iso = on ? 1.f / a.old_std[k] : 1.f;
  const float sr = sd * iso;
  const float vrat = sr * sr, lvrat = logf(vrat);
  double s_kl = 0.0, s_cnt = 0.0, s_ra = 0.0, s_dk = 0.0, s_dp = 0.0;
  const int64_t wave_g = (int64_t)blockIdx.x * 4 + wave, nwaves = (int64_t)gridDim.x * 4;
  for (int64_t r0 = wave_g * rpw; r0 < a.B; r0 += nwaves * rpw) {
    const int64_t r = r0 + sub;
    const bool rv = r < a.B;
    const int64_t rr = rv ? r : a.B - 1;
    const float mu = on ? a.mean[rr * A + k] : 0.f;
    const float ac = on ? a.act[rr * A + k] : 0.f;
    const float dif = ac - mu;
    const float term = on ? -(dif * dif) * (0.5f * ivar) - ls - LOG_SQRT_2PI : 0.f;
    const float lp = group_sum_f(term, G);
    const float dm = on ? (mu - a.old_mean[rr * A + k]) * iso : 0.f;
    const float kl = group_sum_f(on ? 0.5f * (vrat + dm * dm - 1.f - lvrat) : 0.f, G);
    const float ad = a.adv[rr];
    const float ratio = __expf(lp - a.logp_old[rr]);
    const float ind = (kl <= a.p0) ? 1.f : 0.f;
    const float dlp = -(a.p1 * ad * ratio) * a.inv_n;
    const float wk = ind * a.inv_n;
    if (rv && k == 0) { s_kl += (double)(ind * kl); s_cnt += (double)ind; s_ra += (double)(ratio * ad); }
    if (rv && on) {
      const float z = dif * ivar;
      a.d_mean[r * A + k] = wk * dm * iso;
      d_mean_pg[r * A + k] = dlp * z;
      s_dk += (double)(wk * (vrat - 1.f));
      s_dp += (double)(dlp * (dif * z - 1.f));
    }
  }
  s_kl = wave_sum_d(s_kl); s_cnt = wave_sum_d(s_cnt); s_ra = wave_sum_d(s_ra);
  s_dk = stride_sum_d(s_dk, G); s_dp = stride_sum_d(s_dp, G);
  if (lane == 0) { red[wave][0] = s_kl; red[wave][1] = s_cnt; red[wave][2] = s_ra; }
  if (lane < G && lane < A) { red[wave][3 + lane] = s_dk; red[wave][3 + A + lane] = s_dp; }
  __syncthreads();
  if (tid < 3 + 2 * A) a.partial[(int64_t)blockIdx.x * WAS_NS + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}
// sums (float, the layout of spo_kl_penalty_grad's): [0], [1] = 0 (the wide path's critic losses stay in its loss log), [2] count,
// [3] sum ind*KL, [4] sum ratio*adv, [5] rows; d(log_std) KL / PG parts into their gradient buffers
__global__ void wide_klpen_split_finish_kernel(const double* __restrict__ partial, int nblocks, int A, int64_t rows,
                                               float* __restrict__ sums, float* __restrict__ d_ls_kl, float* __restrict__ d_ls_pg) {
  const int k = threadIdx.x;
  if (k >= 3 + 2 * A) return;
  double s = 0.0;
  for (int b = 0; b < nblocks; ++b) s += partial[(int64_t)b * WAS_NS + k];
  if (k == 0) { sums[3] = (float)s; sums[0] = 0.f; sums[1] = 0.f; sums[5] = (float)rows; }
  else if (k == 1) sums[2] = (float)s;
  else if (k == 2) sums[4] = (float)s;
  else if (k < 3 + A) d_ls_kl[k - 3] = (float)s;
  else d_ls_pg[k - 3 - A] = (float)s;
}
// after the all-reduce: grad[begin, n) *= scale with grad[actor_begin, n) += F * pg[actor_begin, n) first, F = sums[2] / sums[5];
// loss_out = the global minibatch's actor loss
__global__ __launch_bounds__(256) void wide_klpen_combine_kernel(float* __restrict__ g, const float* __restrict__ pg,
                                                                 const float* __restrict__ sums, int64_t begin, int64_t actor_begin,
                                                                 int64_t n, float scale, float pg_coef, float* __restrict__ loss_out) {
  const float frac = sums[2] / sums[5];
  for (int64_t i = begin + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    float v = g[i];
    if (i >= actor_begin) v = v + frac * pg[i];
    g[i] = v * scale;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && loss_out) loss_out[0] = (sums[3] - pg_coef * frac * sums[4]) / sums[5];
}

__global__ __launch_bounds__(256) void wide_critic_loss_kernel(const float* __restrict__ v_r, const float* __restrict__ v_c,
                                                               const float* __restrict__ tgt_r, const float* __restrict__ tgt_c, int64_t B,
                                                               float inv_n, float* __restrict__ d_vr, float* __restrict__ d_vc,
                                                               double* __restrict__ partial, float* __restrict__ losses) {
  // losses: given for a one-workgroup launch, which finishes the sums itself (see wide_ppo_loss_kernel)
  __shared__ double red[4][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double a0 = 0.0, a1 = 0.0;
  for (int64_t r = (int64_t)blockIdx.x * 256 + tid; r < B; r += (int64_t)gridDim.x * 256) {
    const float dr = v_r[r] - tgt_r[r], dc = v_c[r] - tgt_c[r];
    a0 += (double)(dr * dr); a1 += (double)(dc * dc);
    d_vr[r] = 2.f * dr * inv_n; d_vc[r] = 2.f * dc * inv_n;
  }
  a0 = wave_sum_d(a0); a1 = wave_sum_d(a1);
  if (lane == 0) { red[wave][0] = a0; red[wave][1] = a1; }
  __syncthreads();
  if (tid < 2) {
    const double v = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
    partial[(int64_t)blockIdx.x * 2 + tid] = v;
    if (losses) losses[tid] = (float)((0.0 + v) / (double)B);
  }
}
__global__ void wide_critic_loss_finish_kernel(const double* __restrict__ partial, int nblocks, int64_t B, float* __restrict__ losses) {
  const int k = threadIdx.x;
  if (k >= 2) return;
  double s = 0.0;
  for (int b = 0; b < nblocks; ++b) s += partial[(int64_t)b * 2 + k];
  losses[k] = (float)(s / (double)B);
}

__global__ __launch_bounds__(256) void wide_fvp_cot_kernel(const float* __restrict__ jv, const float* __restrict__ log_std, int64_t B, int A,
                                                           float inv_ma, float* __restrict__ d_mean) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < B * A; i += (int64_t)gridDim.x * 256) {
    const float sd = expf(log_std[i % A]);
    d_mean[i] = jv[i] * (1.f / (sd * sd)) * inv_ma;
  }
}

struct WlsArgs {
  const float* mean; const float* log_std; const float* act; const float* logp_old; const float* adv_a; const float* adv_b;
  const float* mean_old; const float* log_std_old; int64_t B; int A, G; double* partial;
};
__global__ __launch_bounds__(256) void wide_linesearch_kernel(WlsArgs a) {
  __shared__ double red[4][3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int A = a.A, G = a.G, k = lane & (G - 1), sub = lane / G, rpw = 64 / G;
  const bool on = k < A;
  const float lsv = on ? a.log_std[k] : 0.f;
  const float sdn = expf(lsv), sdo = on ? expf(a.log_std_old[k]) : 1.f;
  const float ivar = 1.f / (sdn * sdn), lsd = on ? logf(sdn) + LOG_SQRT_2PI : 0.f;
  const float sr = sdo / sdn, vr = sr * sr, lvr = logf(vr);
  double s_a = 0.0, s_b = 0.0, s_kl = 0.0;
  const int64_t wave_g = (int64_t)blockIdx.x * 4 + wave, nwaves = (int64_t)gridDim.x * 4;
  for (int64_t r0 = wave_g * rpw; r0 < a.B; r0 += nwaves * rpw) {
    const int64_t r = r0 + sub;
    const bool rv = r < a.B;
    const int64_t rr = rv ? r : a.B - 1;
    const float mu = on ? a.mean[rr * A + k] : 0.f;
    const float dif = (on ? a.act[rr * A + k] : 0.f) - mu;
    const float lp = group_sum_f(on ? -(dif * dif) * (0.5f * ivar) - lsd : 0.f, G);
    const float ratio = expf(lp - a.logp_old[rr]);
    if (rv && on) {
      const float dm = (a.mean_old[rr * A + k] - mu) / sdn;
      s_kl += (double)(0.5f * (vr + dm * dm - 1.f - lvr));
    }
    if (rv && k == 0) { s_a += (double)(ratio * a.adv_a[rr]); s_b += (double)(ratio * a.adv_b[rr]); }
  }
  s_a = wave_sum_d(s_a); s_b = wave_sum_d(s_b); s_kl = wave_sum_d(s_kl);
  if (lane == 0) { red[wave][0] = s_a; red[wave][1] = s_b; red[wave][2] = s_kl; }
  __syncthreads();
  if (tid < 3) a.partial[(int64_t)blockIdx.x * 3 + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}
__global__ void wide_sum3_kernel(const double* __restrict__ partial, int n, double* __restrict__ out, int accumulate) {
  if (threadIdx.x < 3) {
    double s = accumulate ? out[threadIdx.x] : 0.0;
    for (int b = 0; b < n; ++b) s += partial[(int64_t)b * 3 + threadIdx.x];
    out[threadIdx.x] = s;
  }
}

// ---- optimiser step
// Joint clip + Adam over the flat vector of all three networks: stage 1 adds the critics' L2 gradient (2 l2 p) and the value
// coefficient in place and reduces ||g||^2 and the critics' sum p^2; stage 2 forms the clip coefficient; stage 3 is Adam.
struct WideAdamArgs {
  float* theta; float* grad; float* m; float* v; int64_t P, r_end, c_end, actor_begin;
  float l2, vcoef_r, max_norm, lr_actor, lr_critic, b1, b2, eps;
  float w1, w2;                      // 1 - beta1, 1 - beta2 formed on the host in double (csrc/adam_host.h)
  double b1d, b2d;                   // the betas the caller meant: the optimiser clocks are their powers
  double pow_b1, pow_b2;
  double* partial; float* scal;      // scal: {coef, l2 * sum p^2 (reward critic), l2 * sum p^2 (cost critic), ||g||}
  float* losses3;
};
// (the bodies of the optimiser's kernels are shared by the stand-alone kernels -- `a` their kernel argument -- and the table-driven
//  ones below -- `a` a run's entry of a device table)
__device__ __forceinline__ void wide_prep_body(const WideAdamArgs a) {
  __shared__ double red[4][3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double gs = 0.0, pr = 0.0, pc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < a.P; i += (int64_t)gridDim.x * 256) {
    float g = a.grad[i];
    if (i < a.c_end) {
      const float p = a.theta[i];
      g = fmaf(2.f * a.l2, p, g);
      if (i < a.r_end) { g *= a.vcoef_r; pr += (double)(p * p); } else pc += (double)(p * p);
      a.grad[i] = g;
    }
    gs += (double)(g * g);
  }
  gs = wave_sum_d(gs); pr = wave_sum_d(pr); pc = wave_sum_d(pc);
  if (lane == 0) { red[wave][0] = gs; red[wave][1] = pr; red[wave][2] = pc; }
  __syncthreads();
  if (tid < 3) a.partial[(int64_t)blockIdx.x * 3 + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}
__global__ __launch_bounds__(256) void wide_prep_kernel(WideAdamArgs a) { wide_prep_body(a); }
// pow4 (optional): the device-resident optimiser clocks {beta1^t, beta2^t of the critics, of the actor}; the clocks named by
// adv_critics / adv_actor advance here, between the norm and the Adam pass (spo_wide_clip_adam_dev)
// loss_log / log_src / cursor (optional, device): the step's three losses log_src[0..2] are stored at loss_log[3 * (*cursor / cursor_step)] and
// *cursor advances by cursor_step -- the window spo_gather_rows_at reads; a replayed step then needs no host copy in or out
__device__ __forceinline__ void wide_coef_body(const WideAdamArgs a, int nblocks, double* pow4, int adv_critics, int adv_actor,
                                               float* loss_log, const float* log_src, int64_t* cursor, int64_t cursor_step) {
  // one wave: lane l adds the partials l, l + 64, ... in order, then a fixed butterfly over the lanes
  double gs = 0.0, pr = 0.0, pc = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += 64) { gs += a.partial[b * 3]; pr += a.partial[b * 3 + 1]; pc += a.partial[b * 3 + 2]; }
  gs = wave_sum_d(gs); pr = wave_sum_d(pr); pc = wave_sum_d(pc);
  if (threadIdx.x != 0) return;
  if (pow4) {
    if (adv_critics) { pow4[0] *= a.b1d; pow4[1] *= a.b2d; }
    if (adv_actor) { pow4[2] *= a.b1d; pow4[3] *= a.b2d; }
  }
  const float norm = sqrtf((float)gs);
  float coef = a.max_norm / (norm + 1e-6f);                   // clip_grad_norm_ (torch): eps 1e-6
  a.scal[0] = coef > 1.f ? 1.f : coef;
  a.scal[1] = a.l2 * (float)pr; a.scal[2] = a.l2 * (float)pc; a.scal[3] = norm;
  if (a.losses3) { a.losses3[0] += a.scal[1]; a.losses3[1] += a.scal[2]; }      // logged critic losses include their L2 terms
  if (cursor) {
    const int64_t at = cursor[0];
    if (loss_log && log_src) {
      float* row = loss_log + 3 * (at / cursor_step);
      row[0] = log_src[0]; row[1] = log_src[1]; row[2] = log_src[2];
    }
    cursor[0] = at + cursor_step;
  }
}
__global__ __launch_bounds__(64) void wide_coef_kernel(WideAdamArgs a, int nblocks, double* pow4 = nullptr, int adv_critics = 0,
                                                       int adv_actor = 0, float* loss_log = nullptr, const float* log_src = nullptr,
                                                       int64_t* cursor = nullptr, int64_t cursor_step = 0) {
  wide_coef_body(a, nblocks, pow4, adv_critics, adv_actor, loss_log, log_src, cursor, cursor_step);
}
// prep over a sub-range for the joint norm: CUP's second stage clips over the ACTOR's parameters only (cup.py:385)
__device__ __forceinline__ void wide_prep_range_body(const WideAdamArgs a, int64_t n0, int64_t n1) {
  __shared__ double red[4][3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double gs = 0.0;
  for (int64_t i = n0 + (int64_t)blockIdx.x * 256 + tid; i < n1; i += (int64_t)gridDim.x * 256) {
    const float g = a.grad[i];
    gs += (double)(g * g);
  }
  gs = wave_sum_d(gs);
  if (lane == 0) { red[wave][0] = gs; red[wave][1] = 0.0; red[wave][2] = 0.0; }
  __syncthreads();
  if (tid < 3) a.partial[(int64_t)blockIdx.x * 3 + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}
__global__ __launch_bounds__(256) void wide_prep_range_kernel(WideAdamArgs a, int64_t n0, int64_t n1) { wide_prep_range_body(a, n0, n1); }
// clip + Adam with a sub-range: the joint norm spans [norm_begin, P) (wide_prep_kernel, or wide_prep_range_kernel when
// norm_begin != 0); Adam touches [adam_begin, adam_end) only, with the critics' clock below actor_begin and the actor's above;
// outside that range the (stale) gradient is multiplied by the clip coefficient in place when scale_rest != 0.
struct WideAdamExArgs {
  WideAdamArgs b; int64_t adam_begin, adam_end; int scale_rest; double pow_b1_a, pow_b2_a;
};
// DEV_CLOCKS = false: the clocks beta^t BEFORE this step come from the host (b.pow_b1 / b.pow_b2: the critics', pow_b1_a /
// pow_b2_a: the actor's) and advance here; pow4 is not read.
// DEV_CLOCKS = true: pow4 holds the device-resident clocks, already advanced by wide_coef_kernel, and the learning rates.
// MULTI (the table-driven form below): `arg` is a device table of WideOptEntry, run blockIdx.y's x and pow4 are read from its entry.
struct WideOptEntry;
template <bool MULTI> struct WideKernArg {
  typedef WideAdamExArgs AdamEx;
  static __device__ __forceinline__ const WideAdamExArgs& ex(const WideAdamExArgs& x) { return x; }
};
template <> struct WideKernArg<true> {
  typedef const WideOptEntry* __restrict__ AdamEx;
  static __device__ __forceinline__ const WideAdamExArgs& ex(const WideOptEntry* __restrict__ t);
  static __device__ __forceinline__ bool active(const WideOptEntry* __restrict__ t);
  static __device__ __forceinline__ const double* pow4(const WideOptEntry* __restrict__ t);
};
template <bool DEV_CLOCKS, bool MULTI = false>
__global__ __launch_bounds__(256) void wide_adam_kernel(typename WideKernArg<MULTI>::AdamEx arg, const double* __restrict__ pow4) {
  if constexpr (MULTI) {
    if (!WideKernArg<true>::active(arg)) return;
    pow4 = WideKernArg<true>::pow4(arg);
  }
  const WideAdamExArgs x = WideKernArg<MULTI>::ex(arg);   // (a copy: the stand-alone kernel's code is then what it was with `x` its parameter)
  const WideAdamArgs& a = x.b;
  const float coef = a.scal[0];
  float ss_a, ss_c, bc2s_a, bc2s_c;
  if (DEV_CLOCKS) {
    // learning rates: device-resident next to the clocks when set (> 0) -- the actor's follows a per-epoch schedule, and a value baked
    // into a captured launch would make every epoch capture a new graph
    // (a NEGATIVE entry means "take the cfg's": a scheduled or frozen learning rate of exactly 0 is honoured -- ABI 2)
    const float lr_a = pow4[4] >= 0.0 ? (float)pow4[4] : a.lr_actor, lr_c = pow4[5] >= 0.0 ? (float)pow4[5] : a.lr_critic;
    adam_scalars(lr_a, pow4[2], pow4[3], ss_a, bc2s_a);                 // pow4 already advanced: beta^(t+1)
    adam_scalars(lr_c, pow4[0], pow4[1], ss_c, bc2s_c);
  } else {
    adam_scalars(a.lr_actor, x.pow_b1_a * a.b1d, x.pow_b2_a * a.b2d, ss_a, bc2s_a);
    adam_scalars(a.lr_critic, a.pow_b1 * a.b1d, a.pow_b2 * a.b2d, ss_c, bc2s_c);
  }
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.P; i += (int64_t)gridDim.x * 256) {
    if (i >= x.adam_begin && i < x.adam_end) {
      const bool act = i >= a.actor_begin;
      const AdamOut o = adam1(a.theta[i], a.grad[i] * coef, a.m[i], a.v[i], a.b2, a.w1, a.w2, a.eps, act ? ss_a : ss_c, act ? bc2s_a : bc2s_c);
      a.theta[i] = o.p; a.m[i] = o.m; a.v[i] = o.v;
    } else if (x.scale_rest) {
      a.grad[i] = a.grad[i] * coef;
    }
  }
}

// ---- the table-driven (seed-batched) form of the three launches with device-resident clocks (csrc/wide_opt.h): run blockIdx.y of
// S independent runs reads what its stand-alone launches receive as kernel arguments from its entry of a device table (uniform
// index, const __restrict__: scalar loads) and runs the same body on the stand-alone blockIdx.x / gridDim.x.  No block waits for
// another; a block of a run with active == 0 returns after reading `active` and nothing else.
struct WideOptEntry {
  WideAdamExArgs x;
  int64_t norm_begin;                // the joint norm spans [norm_begin, x.b.P): wide_prep_kernel's pass at 0, else wide_prep_range_kernel's
  double* pow4;
  float* loss_log; const float* log_src; int64_t* cursor; int64_t cursor_step;
  int nblocks, adv_critics, adv_actor;
  int active;
};
static_assert(sizeof(WideOptEntry) % 8 == 0, "WideOptEntry: entries are laid out back to back behind another table");
__global__ __launch_bounds__(256) void wide_prep_multi_kernel(const WideOptEntry* __restrict__ tab) {
  if (!tab[blockIdx.y].active) return;
  wide_prep_body(tab[blockIdx.y].x.b);
}
__global__ __launch_bounds__(256) void wide_prep_range_multi_kernel(const WideOptEntry* __restrict__ tab) {
  if (!tab[blockIdx.y].active) return;
  const WideOptEntry& e = tab[blockIdx.y];
  wide_prep_range_body(e.x.b, e.norm_begin, e.x.b.P);
}
__global__ __launch_bounds__(64) void wide_coef_multi_kernel(const WideOptEntry* __restrict__ tab) {
  if (!tab[blockIdx.y].active) return;
  const WideOptEntry& e = tab[blockIdx.y];
  wide_coef_body(e.x.b, e.nblocks, e.pow4, e.adv_critics, e.adv_actor, e.loss_log, e.log_src, e.cursor, e.cursor_step);
}
__device__ __forceinline__ const WideAdamExArgs& WideKernArg<true>::ex(const WideOptEntry* __restrict__ t) { return t[blockIdx.y].x; }
__device__ __forceinline__ bool WideKernArg<true>::active(const WideOptEntry* __restrict__ t) { return t[blockIdx.y].active != 0; }
__device__ __forceinline__ const double* WideKernArg<true>::pow4(const WideOptEntry* __restrict__ t) { return t[blockIdx.y].pow4; }

int64_t wide_opt_blocks(int64_t n_params) {
  const int64_t blocks = (n_params + 255) / 256;
  return blocks > 1024 ? 1024 : blocks;
}
// The checks and the kernel arguments of a clip + Adam step, in ONE place for the four spo_wide_clip_adam* entry points
// (wide_clip_adam) and for every run of a seed-batched table (spo::wide_opt_fill).  `who` names the caller in the messages.
// No HIP call.
int wide_fill_opt(const char* who, float* theta, float* grad, float* adam_m, float* adam_v, int64_t n_params, int64_t reward_critic_end,
                  int64_t cost_critic_end, int64_t actor_begin, const spo_ppo_cfg* cfg, bool dev_clocks, int64_t step_critics,
                  int64_t step_actor, double* pow4_dev, int64_t adam_begin, int64_t adam_end, int64_t norm_begin, int scale_rest,
                  float* losses3_inout, float* scalars4_out, double* partial_ws, int partial_capacity, float* loss_log_dev,
                  const float* log_src_dev, int64_t* cursor_dev, int64_t cursor_step, WideOptEntry* out) {
  SPO_REQUIRE(theta && grad && adam_m && adam_v && cfg && scalars4_out && partial_ws && n_params > 0 &&
                  (dev_clocks ? pow4_dev != nullptr : (step_critics >= 0 && step_actor >= 0)), "%s: bad args", who);
  SPO_REQUIRE(0 <= reward_critic_end && reward_critic_end <= cost_critic_end && cost_critic_end <= actor_begin && actor_begin <= n_params,
              "%s: parameter ranges out of order", who);
  SPO_REQUIRE(0 <= adam_begin && adam_begin <= adam_end && adam_end <= n_params && 0 <= norm_begin && norm_begin <= n_params,
              "%s: optimiser range out of order", who);
  const int64_t blocks = wide_opt_blocks(n_params);
  SPO_REQUIRE((int64_t)partial_capacity >= blocks * 3, "%s: partial workspace too small", who);
  double b1 = 0.0, b2 = 0.0;          // the betas the caller meant (csrc/adam_host.h): clocks and weights both come from them
  float w1, w2;
  SPO_REQUIRE(adam_beta_host(cfg->beta1, &b1, &w1) && adam_beta_host(cfg->beta2, &b2, &w2), "%s: betas (%g, %g) outside [0, 1)", who,
              (double)cfg->beta1, (double)cfg->beta2);
  const WideAdamArgs a{theta, grad, adam_m, adam_v, n_params, reward_critic_end, cost_critic_end, actor_begin,
                       cfg->use_critic_norm ? cfg->l2_coef : 0.f, cfg->use_value_coefficient ? 2.f : 1.f, cfg->max_grad_norm, cfg->lr_actor,
                       cfg->lr_critic, cfg->beta1, cfg->beta2, cfg->adam_eps, w1, w2, b1, b2, dev_clocks ? 1.0 : pow(b1, (double)step_critics),
                       dev_clocks ? 1.0 : pow(b2, (double)step_critics), partial_ws, scalars4_out, losses3_inout};
  *out = WideOptEntry{};
  out->x = WideAdamExArgs{a, adam_begin, adam_end, scale_rest, dev_clocks ? 1.0 : pow(b1, (double)step_actor),
                          dev_clocks ? 1.0 : pow(b2, (double)step_actor)};
  out->norm_begin = norm_begin;
  out->pow4 = dev_clocks ? pow4_dev : (double*)nullptr;
  out->loss_log = loss_log_dev; out->log_src = log_src_dev; out->cursor = cursor_dev; out->cursor_step = cursor_step;
  out->nblocks = (int)blocks;
  // the clocks of the optimisers inside [adam_begin, adam_end) advance on the device
  out->adv_critics = dev_clocks && adam_begin < actor_begin ? 1 : 0;
  out->adv_actor = dev_clocks && adam_end > actor_begin ? 1 : 0;
  out->active = 1;
  return 0;
}

// The one host sequence behind the four spo_wide_clip_adam* entry points: checks, prep -> coefficient -> Adam.  `entry` names the
// caller in the messages (without its spo_ prefix).  pow4_dev == nullptr: host clocks step_critics / step_actor; else the
// device-resident clocks, and loss_log_dev / log_src_dev / cursor_dev / cursor_step as wide_coef_kernel takes them.
int wide_clip_adam(const char* entry, float* theta, float* grad, float* adam_m, float* adam_v, int64_t n_params,
                   int64_t reward_critic_end, int64_t cost_critic_end, int64_t actor_begin, const spo_ppo_cfg* cfg, bool dev_clocks,
                   int64_t step_critics, int64_t step_actor, double* pow4_dev, int64_t adam_begin, int64_t adam_end, int64_t norm_begin,
                   int scale_rest, float* losses3_inout, float* scalars4_out, double* partial_ws, int partial_capacity,
                   float* loss_log_dev, const float* log_src_dev, int64_t* cursor_dev, int64_t cursor_step, void* stream) {
  WideOptEntry e;
  if (int rc = wide_fill_opt(entry + 4, theta, grad, adam_m, adam_v, n_params, reward_critic_end, cost_critic_end, actor_begin, cfg,
                             dev_clocks, step_critics, step_actor, pow4_dev, adam_begin, adam_end, norm_begin, scale_rest, losses3_inout,
                             scalars4_out, partial_ws, partial_capacity, loss_log_dev, log_src_dev, cursor_dev, cursor_step, &e))
    return rc;
  const WideAdamArgs& a = e.x.b;
  const unsigned blocks = (unsigned)e.nblocks;
  hipStream_t st = (hipStream_t)stream;
  if (norm_begin == 0) hipLaunchKernelGGL(wide_prep_kernel, dim3(blocks), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(wide_prep_range_kernel, dim3(blocks), dim3(256), 0, st, a, norm_begin, n_params);
  hipLaunchKernelGGL(wide_coef_kernel, dim3(1), dim3(64), 0, st, a, e.nblocks, e.pow4, e.adv_critics, e.adv_actor, loss_log_dev, log_src_dev,
                     cursor_dev, cursor_step);
  if (dev_clocks) hipLaunchKernelGGL(wide_adam_kernel<true>, dim3(blocks), dim3(256), 0, st, e.x, (const double*)pow4_dev);
  else hipLaunchKernelGGL(wide_adam_kernel<false>, dim3(blocks), dim3(256), 0, st, e.x, (const double*)nullptr);
  SPO_LAUNCH_CHECK(entry);
  return 0;
}

}  // namespace

// ---- csrc/wide_opt.h: the table-driven optimiser launches for callers in other files
size_t spo::wide_opt_entry_bytes() { return sizeof(WideOptEntry); }
int spo::wide_opt_fill(const char* entry, void* entry_out, float* theta, float* grad, float* adam_m, float* adam_v, int64_t n_params,
                       int64_t reward_critic_end, int64_t cost_critic_end, int64_t actor_begin, const spo_ppo_cfg* cfg, double* pow4_dev,
                       int64_t adam_begin, int64_t adam_end, int64_t norm_begin, int scale_rest, float* losses3_inout,
                       float* scalars4_out, double* partial_ws, int partial_capacity, float* loss_log_dev, const float* log_src_dev,
                       int64_t* cursor_dev, int64_t cursor_step) {
  return wide_fill_opt(entry, theta, grad, adam_m, adam_v, n_params, reward_critic_end, cost_critic_end, actor_begin, cfg, true, 0, 0,
                       pow4_dev, adam_begin, adam_end, norm_begin, scale_rest, losses3_inout, scalars4_out, partial_ws, partial_capacity,
                       loss_log_dev, log_src_dev, cursor_dev, cursor_step, static_cast<WideOptEntry*>(entry_out));
}
void spo::wide_opt_launch_multi(const void* entries_dev, int n_replicas, int64_t n_params, int64_t norm_begin, hipStream_t st) {
  const WideOptEntry* tab = static_cast<const WideOptEntry*>(entries_dev);
  const dim3 grid((unsigned)wide_opt_blocks(n_params), (unsigned)n_replicas);
  if (norm_begin == 0) hipLaunchKernelGGL(wide_prep_multi_kernel, grid, dim3(256), 0, st, tab);
  else hipLaunchKernelGGL(wide_prep_range_multi_kernel, grid, dim3(256), 0, st, tab);
  hipLaunchKernelGGL(wide_coef_multi_kernel, dim3(1, (unsigned)n_replicas), dim3(64), 0, st, tab);
  hipLaunchKernelGGL((wide_adam_kernel<true, true>), grid, dim3(256), 0, st, tab, (const double*)nullptr);
}

// ==================================================================================================================== C ABI
extern "C" int64_t spo_mlp_param_count(const spo_mlp_net* net) {
  MlpLay L;
  if (mlp_lay(net, &L)) return -1;
  return L.count();
}
extern "C" int64_t spo_mlp_workspace_floats(const spo_mlp_net* net, int64_t rows) {
  MlpLay L;
  if (mlp_lay(net, &L) || rows < 1) return -1;
  return L.act_off(L.n, rows);
}
extern "C" int64_t spo_mlp_backward_scratch_floats(const spo_mlp_net* net, int64_t rows) {
  MlpLay L;
  if (mlp_lay(net, &L) || rows < 1) return -1;
  int64_t slices = 0;
  for (int l = 0; l < L.n; ++l) {
    const int64_t s = (int64_t)dw_splits(rows, L.d[l + 1], L.d[l]) * L.d[l + 1] * L.d[l];
    slices = s > slices ? s : slices;
  }
  return 2 * rows * (int64_t)L.maxdim() + slices + (int64_t)CS_SLICES * L.maxdim();
}

extern "C" int spo_mlp_forward(const float* theta, const spo_mlp_net* net, const float* x, int64_t rows, float* ws, void* stream) {
  MlpLay L;
  if (int rc = mlp_lay(net, &L)) return rc;
  SPO_REQUIRE(theta && x && ws && rows > 0, "mlp_forward: bad args");
  hipStream_t st = (hipStream_t)stream;
  if (spo::mlp_small_ok(net, rows)) {
    // up to 128 rows: the whole network in one launch (csrc/mlp_small.hip)
    spo::MlpSmallBatch batch;
    batch.count = 1;
    spo::mlp_small_args(theta, net, x, rows, ws, nullptr, nullptr, &batch.a[0]);
    if (int rc = spo::mlp_small_launch(false, batch, st)) return rc;
    SPO_LAUNCH_CHECK("spo_mlp_forward");
    return 0;
  }
  const float* in = x;
  for (int l = 0; l < L.n; ++l) {
    float* out = ws + L.act_off(l, rows);
    const int K = L.d[l], N = L.d[l + 1];
    if (gemm128_ok(in, rows, K, N, false)) {
      // bias + tanh fused into the GEMM epilogue
      hipLaunchKernelGGL(gemm128_kernel<false>, dim3((unsigned)((rows + G2_T - 1) / G2_T), (unsigned)((N + G2_T - 1) / G2_T)), dim3(256), 0, st,
                         in, theta + L.w(l), out, rows, K, N, theta + L.b(l), l + 1 < L.n ? 1 : 0, (const float*)nullptr, w_is_vec(theta + L.w(l)));
    } else {
      if (int rc = gemm_xwT(st, in, theta + L.w(l), out, rows, K, N)) return rc;
      const int64_t n = rows * (int64_t)N;
      hipLaunchKernelGGL(mlp_bias_act_kernel, dim3(ew_grid(n)), dim3(256), 0, st, out, theta + L.b(l), n, N, l + 1 < L.n ? 1 : 0);
    }
    in = out;
  }
  SPO_LAUNCH_CHECK("spo_mlp_forward");
  return 0;
}

extern "C" int spo_mlp_backward(const float* theta, const spo_mlp_net* net, const float* x, int64_t rows, const float* ws,
                                const float* d_out, float* grad, float* scratch, void* stream) {
  MlpLay L;
  if (int rc = mlp_lay(net, &L)) return rc;
  SPO_REQUIRE(theta && x && ws && d_out && grad && scratch && rows > 0, "mlp_backward: bad args");
  hipStream_t st = (hipStream_t)stream;
  if (spo::mlp_small_ok(net, rows)) {
    spo::MlpSmallBatch batch;
    batch.count = 1;
    spo::mlp_small_args(theta, net, x, rows, const_cast<float*>(ws), d_out, grad, &batch.a[0]);
    if (int rc = spo::mlp_small_launch(true, batch, st)) return rc;
    SPO_LAUNCH_CHECK("spo_mlp_backward");
    return 0;
  }
  const int md = L.maxdim();
  float* dA = scratch;                                   // ping-pong dZ buffers
  float* dB = scratch + rows * (int64_t)md;
  float* slices = scratch + 2 * rows * (int64_t)md;
  int64_t smax = 0;
  for (int l = 0; l < L.n; ++l) {
    const int64_t s = (int64_t)dw_splits(rows, L.d[l + 1], L.d[l]) * L.d[l + 1] * L.d[l];
    smax = s > smax ? s : smax;
  }
  float* cs = slices + smax;
  const float* dz = d_out;                               // dZ of the last (linear) layer is d_out itself
  for (int l = L.n - 1; l >= 0; --l) {
    const int N = L.d[l + 1], K = L.d[l];
    const float* hin = l == 0 ? x : ws + L.act_off(l - 1, rows);
    hipLaunchKernelGGL(mlp_colsum_partial_kernel, dim3((N + 255) / 256, CS_SLICES), dim3(256), 0, st, dz, rows, N, cs);
    hipLaunchKernelGGL(mlp_colsum_finish_kernel, dim3((N + 255) / 256), dim3(256), 0, st, cs, N, grad + L.b(l));
    if (int rc = gemm_dyTx(st, dz, hin, grad + L.w(l), rows, K, N, slices)) return rc;
    if (l > 0) {
      float* dh = (dz == dA) ? dB : dA;
      // dH_{l-1} = dZ_l W_l (reduction over this layer's N outputs, K inputs wide) and dZ_{l-1} = dH_{l-1} (1 - h_{l-1}^2)
      if (gemm128_ok(dz, rows, N, K, true)) {
        hipLaunchKernelGGL(gemm128_kernel<true>, dim3((unsigned)((rows + G2_T - 1) / G2_T), (unsigned)((K + G2_T - 1) / G2_T)), dim3(256), 0, st,
                           dz, theta + L.w(l), dh, rows, N, K, (const float*)nullptr, 0, hin, w_is_vec(theta + L.w(l)));
      } else {
        if (int rc = gemm_dyw(st, dz, theta + L.w(l), dh, rows, K, N)) return rc;
        const int64_t n = rows * (int64_t)K;
        hipLaunchKernelGGL(mlp_dtanh_kernel, dim3(ew_grid(n)), dim3(256), 0, st, dh, hin, n);
      }
      dz = dh;
    }
  }
  SPO_LAUNCH_CHECK("spo_mlp_backward");
  return 0;
}

// The same for `count` networks on the same number of rows -- the three networks of a minibatch step -- in ONE launch when every
// network fits the small-row kernel (one workgroup per network), else one call per network.
extern "C" int spo_mlp_forward_multi(int count, const float* const* thetas, const spo_mlp_net* const* nets, const float* const* xs,
                                     int64_t rows, float* const* wss, void* stream) {
  SPO_REQUIRE(count >= 1 && count <= spo::MLP_SMALL_MAX_NETS && thetas && nets && xs && wss && rows > 0, "mlp_forward_multi: bad args");
  bool small = true;
  for (int i = 0; i < count; ++i) {
    SPO_REQUIRE(thetas[i] && nets[i] && xs[i] && wss[i], "mlp_forward_multi: null pointer");
    small = small && spo::mlp_small_ok(nets[i], rows);
  }
  if (!small) {
    for (int i = 0; i < count; ++i)
      if (int rc = spo_mlp_forward(thetas[i], nets[i], xs[i], rows, wss[i], stream)) return rc;
    return 0;
  }
  spo::MlpSmallBatch batch;
  batch.count = count;
  for (int i = 0; i < count; ++i) {
    MlpLay L;
    if (int rc = mlp_lay(nets[i], &L)) return rc;
    spo::mlp_small_args(thetas[i], nets[i], xs[i], rows, wss[i], nullptr, nullptr, &batch.a[i]);
  }
  if (int rc = spo::mlp_small_launch(false, batch, (hipStream_t)stream)) return rc;
  SPO_LAUNCH_CHECK("spo_mlp_forward_multi");
  return 0;
}

extern "C" int spo_mlp_backward_multi(int count, const float* const* thetas, const spo_mlp_net* const* nets, const float* const* xs,
                                      int64_t rows, const float* const* wss, const float* const* d_outs, float* const* grads,
                                      float* const* scratches, void* stream) {
  SPO_REQUIRE(count >= 1 && count <= spo::MLP_SMALL_MAX_NETS && thetas && nets && xs && wss && d_outs && grads && scratches && rows > 0,
              "mlp_backward_multi: bad args");
  bool small = true;
  for (int i = 0; i < count; ++i) {
    SPO_REQUIRE(thetas[i] && nets[i] && xs[i] && wss[i] && d_outs[i] && grads[i] && scratches[i], "mlp_backward_multi: null pointer");
    small = small && spo::mlp_small_ok(nets[i], rows);
  }
  if (!small) {
    for (int i = 0; i < count; ++i)
      if (int rc = spo_mlp_backward(thetas[i], nets[i], xs[i], rows, wss[i], d_outs[i], grads[i], scratches[i], stream)) return rc;
    return 0;
  }
  spo::MlpSmallBatch batch;
  batch.count = count;
  for (int i = 0; i < count; ++i) {
    MlpLay L;
    if (int rc = mlp_lay(nets[i], &L)) return rc;
    spo::mlp_small_args(thetas[i], nets[i], xs[i], rows, const_cast<float*>(wss[i]), d_outs[i], grads[i], &batch.a[i]);
  }
  if (int rc = spo::mlp_small_launch(true, batch, (hipStream_t)stream)) return rc;
  SPO_LAUNCH_CHECK("spo_mlp_backward_multi");
  return 0;
}

extern "C" int64_t spo_mlp_jvp_scratch_floats(const spo_mlp_net* net, int64_t rows) {
  MlpLay L;
  if (mlp_lay(net, &L) || rows < 1) return -1;
  return 2 * rows * (int64_t)L.maxdim();
}
extern "C" int spo_mlp_jvp(const float* theta, const spo_mlp_net* net, const float* tangent, const float* x, int64_t rows,
                           const float* ws, float* dout, float* scratch, void* stream) {
  MlpLay L;
  if (int rc = mlp_lay(net, &L)) return rc;
  SPO_REQUIRE(theta && tangent && x && ws && dout && scratch && rows > 0, "mlp_jvp: bad args");
  hipStream_t st = (hipStream_t)stream;
  const int md = L.maxdim();
  float* bufA = scratch;
  float* bufB = scratch + rows * (int64_t)md;
  const float* dh = nullptr;                      // tangent of the layer input (0 for the observations)
  for (int l = 0; l < L.n; ++l) {
    const int K = L.d[l], N = L.d[l + 1];
    const bool last = l + 1 == L.n;
    const float* hin = l == 0 ? x : ws + L.act_off(l - 1, rows);
    float* y = last ? dout : (dh == bufA ? bufB : bufA);
    // dz_l = h_{l-1} tW_l^T + dh_{l-1} W_l^T + tb_l
    if (int rc = gemm_xwT(st, hin, tangent + L.w(l), y, rows, K, N, 0.f)) return rc;
    if (dh) { if (int rc = gemm_xwT(st, dh, theta + L.w(l), y, rows, K, N, 1.f)) return rc; }
    const int64_t n = rows * (int64_t)N;
    hipLaunchKernelGGL(mlp_jvp_ew_kernel, dim3(ew_grid(n)), dim3(256), 0, st, y, tangent + L.b(l),
                       last ? (const float*)nullptr : ws + L.act_off(l, rows), n, N);
    dh = y;
  }
  SPO_LAUNCH_CHECK("spo_mlp_jvp");
  return 0;
}

extern "C" int spo_gauss_sample(const float* mean, const float* log_std, const float* eps, float* act_out, float* logp_out,
                                int64_t rows, int act_dim, void* stream) {
  SPO_REQUIRE(mean && log_std && act_out && logp_out && rows > 0 && act_dim >= 1 && act_dim <= SPO_WIDE_MAX_ACT, "gauss_sample: bad args");
  hipLaunchKernelGGL(gauss_sample_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, mean, log_std, eps,
                     act_out, logp_out, rows, act_dim);
  SPO_LAUNCH_CHECK("spo_gauss_sample");
  return 0;
}
extern "C" int spo_gauss_kl_sum(const float* mean_old, const float* log_std_old, const float* mean_new, const float* log_std_new,
                                int64_t rows, int act_dim, double* partial_ws, int partial_capacity, double* sum_inout, int accumulate,
                                void* stream) {
  SPO_REQUIRE(mean_old && log_std_old && mean_new && log_std_new && partial_ws && sum_inout && rows > 0 && act_dim >= 1 &&
                  act_dim <= SPO_WIDE_MAX_ACT && partial_capacity >= 1, "gauss_kl_sum: bad args");
  int64_t blocks = (rows + 255) / 256;
  if (blocks > 512) blocks = 512;
  if (blocks > partial_capacity) blocks = partial_capacity;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(gauss_kl_kernel, dim3((unsigned)blocks), dim3(256), 0, st, mean_old, log_std_old, mean_new, log_std_new, rows, act_dim,
                     partial_ws);
  hipLaunchKernelGGL(gauss_kl_finish_kernel, dim3(1), dim3(64), 0, st, partial_ws, (int)blocks, sum_inout, accumulate);
  SPO_LAUNCH_CHECK("spo_gauss_kl_sum");
  return 0;
}

extern "C" int spo_gather_rows_at(int count, const float* const* srcs, const int* widths, float* const* dsts, const int64_t* idx,
                                  const int64_t* cursor_dev, int64_t n, void* stream) {
  SPO_REQUIRE(count >= 1 && count <= SPO_GATHER_MAX && srcs && widths && dsts && idx && n > 0, "gather_rows: bad args");
  GatherArgs a;
  a.count = count; a.idx = idx; a.cursor = cursor_dev; a.n = n;
  int wmax = 1;
  for (int k = 0; k < count; ++k) {
    SPO_REQUIRE(srcs[k] && dsts[k] && widths[k] >= 1, "gather_rows: bad array %d", k);
    a.src[k] = srcs[k]; a.dst[k] = dsts[k]; a.width[k] = widths[k];
    wmax = widths[k] > wmax ? widths[k] : wmax;
  }
  const int64_t blocks = (n * wmax + 255) / 256;
  hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)(blocks > 1024 ? 1024 : blocks), (unsigned)count), dim3(256), 0, (hipStream_t)stream, a);
  SPO_LAUNCH_CHECK("spo_gather_rows");
  return 0;
}
extern "C" int spo_gather_rows(int count, const float* const* srcs, const int* widths, float* const* dsts, const int64_t* idx, int64_t n,
                               void* stream) {
  return spo_gather_rows_at(count, srcs, widths, dsts, idx, nullptr, n, stream);
}

extern "C" int spo_wide_critic_loss(const float* v_r, const float* v_c, const float* tgt_r, const float* tgt_c, int64_t rows,
                                    float* d_vr, float* d_vc, float* losses2, double* partial_ws, int partial_capacity, void* stream) {
  SPO_REQUIRE(v_r && v_c && tgt_r && tgt_c && d_vr && d_vc && losses2 && partial_ws && rows > 0, "wide_critic_loss: bad args");
  int64_t blocks = (rows + 255) / 256;
  if (blocks > 256) blocks = 256;
  SPO_REQUIRE((int64_t)partial_capacity >= blocks * 2, "wide_critic_loss: partial workspace too small");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(wide_critic_loss_kernel, dim3((unsigned)blocks), dim3(256), 0, st, v_r, v_c, tgt_r, tgt_c, rows, 1.f / (float)rows, d_vr,
                     d_vc, partial_ws, blocks == 1 ? losses2 : (float*)nullptr);
  if (blocks > 1) hipLaunchKernelGGL(wide_critic_loss_finish_kernel, dim3(1), dim3(64), 0, st, partial_ws, (int)blocks, rows, losses2);
  SPO_LAUNCH_CHECK("spo_wide_critic_loss");
  return 0;
}

extern "C" int spo_wide_actor_loss(int mode, const float* mean, const float* log_std, const float* act, const float* logp_old,
                                   const float* adv, const float* old_mean, const float* old_std, int64_t rows, int64_t rows_total,
                                   int act_dim, float p0, float p1, float* d_mean, double* sums_inout, int accumulate,
                                   float* loss_out, float* d_log_std_out, double* partial_ws, int partial_capacity, void* stream) {
  SPO_REQUIRE(mode >= WA_CLIP && mode <= WA_KLPEN, "wide_actor_loss: mode %d outside [0,2]", mode);
  SPO_REQUIRE(mean && log_std && act && logp_old && adv && d_mean && sums_inout && partial_ws && rows > 0 && rows_total >= rows,
              "wide_actor_loss: bad args");
  SPO_REQUIRE(act_dim >= 1 && act_dim <= SPO_WIDE_MAX_ACT, "wide_actor_loss: act_dim %d outside [1,%d]", act_dim, SPO_WIDE_MAX_ACT);
  SPO_REQUIRE(mode != WA_KLPEN || (old_mean && old_std), "wide_actor_loss: the KL-penalty loss needs old_mean / old_std");
  const int G = pow2ceil(act_dim);
  const int64_t rpb = 4 * (64 / G);
  int64_t blocks = (rows + rpb - 1) / rpb;
  if (blocks > 256) blocks = 256;
  SPO_REQUIRE((int64_t)partial_capacity >= blocks * WA_NS, "wide_actor_loss: partial workspace too small (%d < %lld)", partial_capacity,
              (long long)(blocks * WA_NS));
  hipStream_t st = (hipStream_t)stream;
  WaArgs a{mean, log_std, act, logp_old, adv, old_mean, old_std, rows, act_dim, G, p0, p1, 1.f / (float)rows_total, sums_inout + 1, d_mean,
           partial_ws};
  float loss_scale = 1.f;
  if (mode == WA_CLIP) {
    hipLaunchKernelGGL(wide_actor_loss_kernel<WA_CLIP>, dim3((unsigned)blocks), dim3(256), 0, st, a);
    loss_scale = -1.f / (float)rows_total;
  } else if (mode == WA_SURR) {
    hipLaunchKernelGGL(wide_actor_loss_kernel<WA_SURR>, dim3((unsigned)blocks), dim3(256), 0, st, a);
    loss_scale = 1.f / (float)rows_total;
  } else {
    // pass 1: the indicator count (the loss couples every row to mean_i(ind_i), focops.py:331); pass 2 reads it from sums[1]
    SPO_REQUIRE(!accumulate && rows == rows_total, "wide_actor_loss: the KL-penalty loss is a minibatch loss (no row chunks)");
    hipLaunchKernelGGL(wide_actor_loss_kernel<WA_KLPEN_COUNT>, dim3((unsigned)blocks), dim3(256), 0, st, a);
    hipLaunchKernelGGL(wide_actor_loss_finish_kernel, dim3(1), dim3(128), 0, st, partial_ws, (int)blocks, 0, sums_inout, 0, 0.f,
                       (float*)nullptr, (float*)nullptr);
    hipLaunchKernelGGL(wide_actor_loss_kernel<WA_KLPEN>, dim3((unsigned)blocks), dim3(256), 0, st, a);
    loss_scale = -1.f / (float)rows_total;
  }
  hipLaunchKernelGGL(wide_actor_loss_finish_kernel, dim3(1), dim3(128), 0, st, partial_ws, (int)blocks, act_dim, sums_inout, accumulate,
                     loss_scale, loss_out, d_log_std_out);
  SPO_LAUNCH_CHECK("spo_wide_actor_loss");
  return 0;
}

extern "C" int spo_wide_ppo_loss(const float* v_r, const float* v_c, const float* mean, const float* log_std, const float* act,
                                 const float* logp_old, const float* adv, const float* tgt_r, const float* tgt_c, int64_t rows,
                                 int act_dim, float clip, float* d_vr, float* d_vc, float* d_mean, float* d_log_std,
                                 float* losses3, double* partial_ws, int partial_capacity, void* stream) {
  SPO_REQUIRE(v_r && v_c && mean && log_std && act && logp_old && adv && tgt_r && tgt_c && d_vr && d_vc && d_mean && d_log_std &&
                  losses3 && partial_ws && rows > 0, "wide_ppo_loss: bad args");
  SPO_REQUIRE(act_dim >= 1 && act_dim <= SPO_WIDE_MAX_ACT, "wide_ppo_loss: act_dim %d outside [1,%d]", act_dim, SPO_WIDE_MAX_ACT);
  if (act_dim > SPO_MAX_ACT) {
    // wider action vectors (HumanoidVelocity: 17): the lanes-per-row actor-loss kernels (wide_actor_loss_kernel);
    // partial_ws = [256 actor rows | 512 critic partials | sums]
    constexpr int64_t need = 256 * (2 + SPO_WIDE_MAX_ACT) + 512 + (2 + SPO_WIDE_MAX_ACT);
    SPO_REQUIRE((int64_t)partial_capacity >= need, "wide_ppo_loss: partial workspace too small (%d < %lld)", partial_capacity, (long long)need);
    double* crit = partial_ws + 256 * (2 + SPO_WIDE_MAX_ACT);
    if (int rc = spo_wide_critic_loss(v_r, v_c, tgt_r, tgt_c, rows, d_vr, d_vc, losses3, crit, 512, stream)) return rc;
    return spo_wide_actor_loss(0, mean, log_std, act, logp_old, adv, nullptr, nullptr, rows, rows, act_dim, clip, 0.f, d_mean, crit + 512, 0,
                               losses3 + 2, d_log_std, partial_ws, 256 * (2 + SPO_WIDE_MAX_ACT), stream);
  }
  int64_t blocks = (rows + 255) / 256;
  if (blocks > 256) blocks = 256;
  SPO_REQUIRE(partial_capacity >= blocks * WL_NS, "wide_ppo_loss: partial workspace too small (%d < %lld)", partial_capacity, (long long)(blocks * WL_NS));
  hipStream_t st = (hipStream_t)stream;
  const bool one = blocks == 1;
  hipLaunchKernelGGL(wide_ppo_loss_kernel, dim3((unsigned)blocks), dim3(256), 0, st, v_r, v_c, mean, log_std, act, logp_old, adv, tgt_r,
                     tgt_c, rows, act_dim, clip, d_vr, d_vc, d_mean, partial_ws, one ? losses3 : (float*)nullptr,
                     one ? d_log_std : (float*)nullptr);
  if (!one) hipLaunchKernelGGL(wide_ppo_loss_finish_kernel, dim3(1), dim3(64), 0, st, partial_ws, (int)blocks, act_dim, rows, losses3, d_log_std);
  SPO_LAUNCH_CHECK("spo_wide_ppo_loss");
  return 0;
}

extern "C" int spo_wide_kl_penalty_split(const float* mean, const float* log_std, const float* act, const float* logp_old,
                                         const float* adv, const float* old_mean, const float* old_std, int64_t rows, int act_dim,
                                         float kl_bound, float pg_coef, float* d_mean_kl, float* d_mean_pg, float* d_log_std_kl,
                                         float* d_log_std_pg, float* sums, double* partial_ws, int partial_capacity, void* stream) {
  SPO_REQUIRE(mean && log_std && act && logp_old && adv && old_mean && old_std && d_mean_kl && d_mean_pg && d_log_std_kl &&
                  d_log_std_pg && sums && partial_ws, "wide_kl_penalty_split: null pointer");
  SPO_REQUIRE(rows > 0, "wide_kl_penalty_split: bad rows %lld", (long long)rows);
  SPO_REQUIRE(act_dim >= 1 && act_dim <= SPO_WIDE_MAX_ACT, "wide_kl_penalty_split: act_dim %d outside [1,%d]", act_dim, SPO_WIDE_MAX_ACT);
  const int G = pow2ceil(act_dim);
  const int64_t rpb = 4 * (64 / G);
  int64_t blocks = (rows + rpb - 1) / rpb;
  if (blocks > 256) blocks = 256;
  SPO_REQUIRE((int64_t)partial_capacity >= blocks * WAS_NS, "wide_kl_penalty_split: partial workspace too small (%d < %lld)",
              partial_capacity, (long long)(blocks * WAS_NS));
  hipStream_t st = (hipStream_t)stream;
  WaArgs a{mean, log_std, act, logp_old, adv, old_mean, old_std, rows, act_dim, G, kl_bound, pg_coef, 1.f / (float)rows, nullptr,
           d_mean_kl, partial_ws};
  hipLaunchKernelGGL(wide_klpen_split_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a, d_mean_pg);
  hipLaunchKernelGGL(wide_klpen_split_finish_kernel, dim3(1), dim3(192), 0, st, partial_ws, (int)blocks, act_dim, rows, sums,
                     d_log_std_kl, d_log_std_pg);
  SPO_LAUNCH_CHECK("spo_wide_kl_penalty_split");
  return 0;
}

extern "C" int spo_wide_kl_penalty_combine(float* grad, const float* pg_grad, const float* sums, int64_t n_params, int64_t begin,
                                           int64_t actor_begin, float grad_scale, float pg_coef, float* loss_out, void* stream) {
  SPO_REQUIRE(grad && pg_grad && sums, "wide_kl_penalty_combine: null pointer");
  SPO_REQUIRE(n_params > 0 && begin >= 0 && begin <= actor_begin && actor_begin < n_params,
              "wide_kl_penalty_combine: bad ranges (begin %lld, actor_begin %lld, n_params %lld)", (long long)begin,
              (long long)actor_begin, (long long)n_params);
  int64_t blocks = (n_params - begin + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(wide_klpen_combine_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, grad, pg_grad, sums, begin,
                     actor_begin, n_params, grad_scale, pg_coef, loss_out);
  SPO_LAUNCH_CHECK("spo_wide_kl_penalty_combine");
  return 0;
}

extern "C" int spo_wide_fvp_cotangent(const float* jv, const float* log_std, int64_t rows, int64_t rows_total, int act_dim,
                                      float* d_mean, void* stream) {
  SPO_REQUIRE(jv && log_std && d_mean && rows > 0 && rows_total >= rows && act_dim >= 1 && act_dim <= SPO_WIDE_MAX_ACT,
              "wide_fvp_cotangent: bad args");
  const float inv_ma = (float)(1.0 / ((double)rows_total * (double)act_dim));
  hipLaunchKernelGGL(wide_fvp_cot_kernel, dim3(ew_grid(rows * act_dim)), dim3(256), 0, (hipStream_t)stream, jv, log_std, rows, act_dim, inv_ma,
                     d_mean);
  SPO_LAUNCH_CHECK("spo_wide_fvp_cotangent");
  return 0;
}

extern "C" int spo_wide_linesearch_sums(const float* mean_new, const float* log_std_new, const float* act, const float* logp_old,
                                        const float* adv_a, const float* adv_b, const float* mean_old, const float* log_std_old,
                                        int64_t rows, int act_dim, double* partial_ws, int partial_capacity, double* sums3_inout,
                                        int accumulate, void* stream) {
  SPO_REQUIRE(mean_new && log_std_new && act && logp_old && adv_a && adv_b && mean_old && log_std_old && partial_ws && sums3_inout &&
                  rows > 0 && act_dim >= 1 && act_dim <= SPO_WIDE_MAX_ACT, "wide_linesearch_sums: bad args");
  const int G = pow2ceil(act_dim);
  const int64_t rpb = 4 * (64 / G);
  int64_t blocks = (rows + rpb - 1) / rpb;
  if (blocks > 512) blocks = 512;
  if (blocks * 3 > partial_capacity) blocks = partial_capacity / 3;
  SPO_REQUIRE(blocks >= 1, "wide_linesearch_sums: partial capacity too small");
  WlsArgs a{mean_new, log_std_new, act, logp_old, adv_a, adv_b, mean_old, log_std_old, rows, act_dim, G, partial_ws};
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(wide_linesearch_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a);
  hipLaunchKernelGGL(wide_sum3_kernel, dim3(1), dim3(64), 0, st, partial_ws, (int)blocks, sums3_inout, accumulate);
  SPO_LAUNCH_CHECK("spo_wide_linesearch_sums");
  return 0;
}

// Joint clip + Adam of a minibatch step: every parameter, one clock (ppo_lag.py:310-329).
extern "C" int spo_wide_clip_adam(float* theta, float* grad, float* adam_m, float* adam_v, int64_t n_params, int64_t reward_critic_end,
                                  int64_t cost_critic_end, int64_t actor_begin, const spo_ppo_cfg* cfg, int64_t adam_step_host,
                                  float* losses3_inout, float* scalars4_out, double* partial_ws, int partial_capacity, void* stream) {
  return wide_clip_adam("spo_wide_clip_adam", theta, grad, adam_m, adam_v, n_params, reward_critic_end, cost_critic_end, actor_begin, cfg,
                        false, adam_step_host, adam_step_host, nullptr, 0, n_params, 0, 0, losses3_inout, scalars4_out, partial_ws,
                        partial_capacity, nullptr, nullptr, nullptr, 0, stream);
}

extern "C" int spo_wide_clip_adam_ex(float* theta, float* grad, float* adam_m, float* adam_v, int64_t n_params, int64_t reward_critic_end,
                                     int64_t cost_critic_end, int64_t actor_begin, const spo_ppo_cfg* cfg, int64_t adam_step_critics_host,
                                     int64_t adam_step_actor_host, int64_t adam_begin, int64_t adam_end, int64_t norm_begin,
                                     int scale_rest, float* losses3_inout, float* scalars4_out, double* partial_ws,
                                     int partial_capacity, void* stream) {
  return wide_clip_adam("spo_wide_clip_adam_ex", theta, grad, adam_m, adam_v, n_params, reward_critic_end, cost_critic_end, actor_begin,
                        cfg, false, adam_step_critics_host, adam_step_actor_host, nullptr, adam_begin, adam_end, norm_begin, scale_rest,
                        losses3_inout, scalars4_out, partial_ws, partial_capacity, nullptr, nullptr, nullptr, 0, stream);
}

// Device-resident optimiser clocks: pow4_dev = double[6] = {beta1^t, beta2^t of the critics' optimisers, beta1^t, beta2^t of the actor's}
// BEFORE this step, then {lr_actor, lr_critic} (negative: take the cfg's).  The clocks of the optimisers inside [adam_begin, adam_end) advance by one step on the device (one thread, between the
// norm and the Adam pass), so the launch sequence of a minibatch step has no host-side argument that changes from step to step and
// can be captured once as a HIP graph and replayed (the wide path at small batches is launch-bound: ~70 launches per step).
extern "C" int spo_wide_clip_adam_dev_log(float* theta, float* grad, float* adam_m, float* adam_v, int64_t n_params, int64_t reward_critic_end,
                                          int64_t cost_critic_end, int64_t actor_begin, const spo_ppo_cfg* cfg, double* pow4_dev,
                                          int64_t adam_begin, int64_t adam_end, int64_t norm_begin, int scale_rest, float* losses3_inout,
                                          float* scalars4_out, double* partial_ws, int partial_capacity, float* loss_log_dev,
                                          const float* log_src_dev, int64_t* cursor_dev, int64_t cursor_step, void* stream) {
  SPO_REQUIRE(!cursor_dev || cursor_step > 0, "wide_clip_adam_dev_log: cursor_step must be > 0");
  return wide_clip_adam("spo_wide_clip_adam_dev", theta, grad, adam_m, adam_v, n_params, reward_critic_end, cost_critic_end, actor_begin,
                        cfg, true, 0, 0, pow4_dev, adam_begin, adam_end, norm_begin, scale_rest, losses3_inout, scalars4_out, partial_ws,
                        partial_capacity, loss_log_dev, log_src_dev, cursor_dev, cursor_step, stream);
}
extern "C" int spo_wide_clip_adam_dev(float* theta, float* grad, float* adam_m, float* adam_v, int64_t n_params, int64_t reward_critic_end,
                                      int64_t cost_critic_end, int64_t actor_begin, const spo_ppo_cfg* cfg, double* pow4_dev,
                                      int64_t adam_begin, int64_t adam_end, int64_t norm_begin, int scale_rest, float* losses3_inout,
                                      float* scalars4_out, double* partial_ws, int partial_capacity, void* stream) {
  return spo_wide_clip_adam_dev_log(theta, grad, adam_m, adam_v, n_params, reward_critic_end, cost_critic_end, actor_begin, cfg, pow4_dev,
                                    adam_begin, adam_end, norm_begin, scale_rest, losses3_inout, scalars4_out, partial_ws, partial_capacity,
                                    nullptr, nullptr, nullptr, 0, stream);
}
