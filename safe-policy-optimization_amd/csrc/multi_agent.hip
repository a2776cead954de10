// Multi-agent (MAPPO-L family) masked GAE with PopArt de-normalisation, gfx950.   [SURVEY.md 8 f3, first piece]
//
// Replaces SeparatedReplayBuffer.compute_returns + compute_cost_returns
// (reference safepo/common/buffer.py:356-384): a Python loop over episode_length with ~10 tiny torch ops per
// step per agent.  Layout is the reference's own: time-major [T+1, N, 1] value/mask arrays, [T, N, 1] rewards.
// One lane per rollout thread walks t = T-1..0 in fp32 with the reference's exact operation order
//     dn(x)  = x * sqrt(var) + mean                               (PopArt.denormalize, popart.py:117-133)
//     delta  = r_t + gamma * dn(v_{t+1}) * mask_{t+1} - dn(v_t)
//     gae    = delta + gamma*lambda * mask_{t+1} * gae
//     ret_t  = gae + dn(v_t)
// so results are BIT-IDENTICAL to the reference; every row access is coalesced across rollout threads.
// HBM-bound: 20 B read (r, c, v_r, v_c, mask) + 8 B written per (thread, step); loads are issued UNROLL steps ahead.
#include "common.h"
#include "../../include/safepo_hip.h"

namespace {

struct MaArgs {
  const float* rewards; const float* costs;       // [T, N]
  const float* value_preds; const float* cost_preds; const float* masks;   // [T+1, N]
  float* returns; float* cost_returns;            // [T+1, N] (row T untouched, as in the reference)
  int64_t T; int64_t N;
  float gamma, gl;                                // gamma, fp32(gamma*lambda formed in double)
  float sd_r, mu_r, sd_c, mu_c;                   // sqrt(var), mean of the two PopArt normalisers
};

template <int UNROLL>
__global__ __launch_bounds__(256) void ma_gae_kernel(MaArgs a) {
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= a.N) return;
  const int64_t N = a.N;
  float gae_r = 0.f, gae_c = 0.f;
  float vn_r = __fadd_rn(__fmul_rn(a.value_preds[a.T * N + n], a.sd_r), a.mu_r);      // dn(v_T)
  float vn_c = __fadd_rn(__fmul_rn(a.cost_preds[a.T * N + n], a.sd_c), a.mu_c);
  float m_next = a.masks[a.T * N + n];
  for (int64_t t0 = a.T - 1; t0 >= 0; t0 -= UNROLL) {
    float r[UNROLL], c[UNROLL], vr[UNROLL], vc[UNROLL], mk[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int64_t t = t0 - u;
      const bool ok = t >= 0;
      const int64_t o = (ok ? t : 0) * N + n;
      r[u] = a.rewards[o]; c[u] = a.costs[o]; vr[u] = a.value_preds[o]; vc[u] = a.cost_preds[o]; mk[u] = a.masks[o];
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int64_t t = t0 - u;
      if (t < 0) break;
      const float dr = __fadd_rn(__fmul_rn(vr[u], a.sd_r), a.mu_r);
      const float dc = __fadd_rn(__fmul_rn(vc[u], a.sd_c), a.mu_c);
      // delta = rewards[t] + gamma * dn(v[t+1]) * masks[t+1] - dn(v[t])          (buffer.py:375)
      const float del_r = __fsub_rn(__fadd_rn(r[u], __fmul_rn(__fmul_rn(a.gamma, vn_r), m_next)), dr);
      const float del_c = __fsub_rn(__fadd_rn(c[u], __fmul_rn(__fmul_rn(a.gamma, vn_c), m_next)), dc);
      // gae = delta + gamma * gae_lambda * masks[t+1] * gae                        (buffer.py:376)
      gae_r = __fadd_rn(del_r, __fmul_rn(__fmul_rn(a.gl, m_next), gae_r));
      gae_c = __fadd_rn(del_c, __fmul_rn(__fmul_rn(a.gl, m_next), gae_c));
      a.returns[t * N + n] = __fadd_rn(gae_r, dr);                                  // buffer.py:377
      a.cost_returns[t * N + n] = __fadd_rn(gae_c, dc);
      vn_r = dr; vn_c = dc; m_next = mk[u];
    }
  }
}

}  // namespace

extern "C" int spo_ma_gae(const float* rewards, const float* costs, const float* value_preds, const float* cost_preds,
                          const float* masks, float* returns, float* cost_returns, int64_t T, int64_t num_threads,
                          double gamma, double gae_lambda, float denorm_std_r, float denorm_mean_r,
                          float denorm_std_c, float denorm_mean_c, void* stream) {
  SPO_REQUIRE(rewards && costs && value_preds && cost_preds && masks && returns && cost_returns, "ma_gae: null pointer");
  SPO_REQUIRE(T >= 0 && num_threads >= 0, "ma_gae: negative size");
  if (T == 0 || num_threads == 0) return 0;
  MaArgs a{rewards, costs, value_preds, cost_preds, masks, returns, cost_returns, T, num_threads,
           (float)gamma, (float)(gamma * gae_lambda), denorm_std_r, denorm_mean_r, denorm_std_c, denorm_mean_c};
  const unsigned blocks = (unsigned)((num_threads + 255) / 256);
  hipLaunchKernelGGL((ma_gae_kernel<8>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
  SPO_LAUNCH_CHECK("spo_ma_gae");
  return 0;
}

// ---------------------------------------------------------------- insert of one environment step into the stacked buffers
// Runner.insert (reference mappolag.py:449-492): per step the runner copies the environment's [N, agents, ...] outputs into
// every agent's time-major buffer and forms masks / active masks from the done flags -- a dozen tiny launches per step whose
// cost is the host's launch time.  One kernel does the six fields: dst(field)[agent][n][:] = src(field)[n][agent][:], with
//     masks[a][n]        = all_a' done[n][a'] ? 0 : 1                                     (mappolag.py:458-463)
//     active_masks[a][n] = done[n][a] && !all-done ? 0 : 1                                (mappolag.py:465-467)
// dst pointers address the (agent 0, step slot) row; agent_stride = floats between two agents' buffers of that field.
namespace {
struct InsArgs {
  const float* obs; const float* share_obs; const float* rewards; const float* costs; const unsigned char* dones;
  float* obs_d; float* share_d; float* rew_d; float* cost_d; float* mask_d; float* act_d;
  int64_t obs_s, share_s, rew_s, cost_s, mask_s, act_s;      // agent strides (floats)
  int64_t N; int A, Do, Ds;
};
__global__ __launch_bounds__(256) void ma_insert_kernel(InsArgs a) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);          // one wave per (n, agent) row
  const int lane = threadIdx.x & 63;
  if (row >= a.N * a.A) return;
  const int64_t n = row / a.A;
  const int ag = (int)(row - n * a.A);
  for (int c = lane; c < a.Do; c += 64) a.obs_d[ag * a.obs_s + n * a.Do + c] = a.obs[row * a.Do + c];
  for (int c = lane; c < a.Ds; c += 64) a.share_d[ag * a.share_s + n * a.Ds + c] = a.share_obs[row * a.Ds + c];
  if (lane == 0) {
    a.rew_d[ag * a.rew_s + n] = a.rewards[row];
    if (a.costs) a.cost_d[ag * a.cost_s + n] = a.costs[row];
    bool all_done = true;
    for (int k = 0; k < a.A; ++k) all_done = all_done && a.dones[n * a.A + k] != 0;
    const bool mine = a.dones[row] != 0;
    a.mask_d[ag * a.mask_s + n] = all_done ? 0.f : 1.f;
    a.act_d[ag * a.act_s + n] = (mine && !all_done) ? 0.f : 1.f;
  }
}
}  // namespace

extern "C" int spo_ma_insert_step(const float* obs, const float* share_obs, const float* rewards, const float* costs,
                                  const unsigned char* dones, float* obs_dst, int64_t obs_agent_stride, float* share_obs_dst,
                                  int64_t share_obs_agent_stride, float* rewards_dst, int64_t rewards_agent_stride, float* costs_dst,
                                  int64_t costs_agent_stride, float* masks_dst, int64_t masks_agent_stride, float* active_masks_dst,
                                  int64_t active_masks_agent_stride, int64_t num_threads, int32_t num_agents, int32_t obs_dim,
                                  int32_t share_obs_dim, void* stream) {
  SPO_REQUIRE(obs && share_obs && rewards && dones && obs_dst && share_obs_dst && rewards_dst && masks_dst && active_masks_dst,
              "ma_insert_step: null pointer");
  SPO_REQUIRE((costs == nullptr) == (costs_dst == nullptr), "ma_insert_step: costs and costs_dst go together");
  SPO_REQUIRE(num_threads > 0 && num_agents > 0 && num_agents <= 64 && obs_dim > 0 && share_obs_dim > 0, "ma_insert_step: bad sizes");
  InsArgs a{obs, share_obs, rewards, costs, dones, obs_dst, share_obs_dst, rewards_dst, costs_dst, masks_dst, active_masks_dst,
            obs_agent_stride, share_obs_agent_stride, rewards_agent_stride, costs_agent_stride, masks_agent_stride,
            active_masks_agent_stride, num_threads, num_agents, obs_dim, share_obs_dim};
  const int64_t rows = num_threads * num_agents;
  const int64_t blocks = (rows + 3) / 4;
  if (blocks > 0x7fffffffLL) return spo::fail(-1, "ma_insert_step: %lld rows exceed the launch grid", (long long)rows);
  hipLaunchKernelGGL(ma_insert_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  SPO_LAUNCH_CHECK("spo_ma_insert_step");
  return 0;
}

// ---------------------------------------------------------------- MACPO line search: the sums of one candidate
// Reference safepo/multi_agent/macpo.py:329-366 up to the accept test.  Per candidate the host-driven form ran the log-prob
// kernel and ~20 torch launches (exp, prod, three means, the KL expression) and read three scalars; here one row pass leaves
//     {sum_r ratio*factor*adv, sum_r ratio*factor*cost_adv, sum_r KL_row, sum_r ratio}
// as fp64 ROW SUMS, which is what a rank of a data-parallel job can add to the other ranks' (the caller divides by the global
// row count).  ratio = prod_d exp(logp_d - old_logp_d) with logp_d exactly as ma_logp_kernel (csrc/ma_net.hip) forms it;
// KL_row = sum_d [log s_old - log s + (s_old^2 + (mu_old - mu)^2) / (1e-8 + 2 s^2) - 0.5]  (macpo.py:153-166, as written).
// Fixed-order reduction: wave shuffle tree -> four waves -> per-block partial -> one workgroup per sum over the partials.
namespace {
constexpr float MA_LOG_SQRT_2PI_F = 0.91893853320467274178f;
constexpr int LS_NS = 4;
constexpr int LS_MAX_BLOCKS = 1024;

__global__ __launch_bounds__(256) void ma_trpo_ls_kernel(
    const float* __restrict__ mean, const float* __restrict__ log_std, float xc, float yc, const float* __restrict__ act,
    const float* __restrict__ old_logp, const float* __restrict__ adv, const float* __restrict__ cost_adv,
    const float* __restrict__ factor, const float* __restrict__ mu_old, const float* __restrict__ std_old,
    float* __restrict__ ratio_out, double* __restrict__ partial, int64_t B, int A) {
  __shared__ double sh[LS_NS][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float sd[SPO_MAX_ACT], so2[SPO_MAX_ACT], dlog[SPO_MAX_ACT];
  for (int a = 0; a < A; ++a) {
    sd[a] = yc / (1.f + expf(-log_std[a] / xc));
    const float so = std_old[a];
    so2[a] = so * so;
    dlog[a] = logf(so) - logf(sd[a]);
  }
  double acc[LS_NS] = {0, 0, 0, 0};
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < B; r += (int64_t)gridDim.x * 256) {
    float ratio = 1.f, kl = 0.f;
    for (int a = 0; a < A; ++a) {
      const float mu = mean[r * A + a];
      const float d = act[r * A + a] - mu;
      const float lp = -(d * d) / (2.f * sd[a] * sd[a]) - logf(sd[a]) - MA_LOG_SQRT_2PI_F;
      ratio *= expf(lp - old_logp[r * A + a]);                 // torch.exp per dimension, then torch.prod
      const float dm = mu_old[r * A + a] - mu;
      kl += dlog[a] + (so2[a] + dm * dm) / (1e-8f + 2.f * sd[a] * sd[a]) - 0.5f;
    }
    const float w = ratio * factor[r];
    acc[0] += (double)(w * adv[r]);
    acc[1] += (double)(w * cost_adv[r]);
    acc[2] += (double)kl;
    acc[3] += (double)ratio;
    if (ratio_out) ratio_out[r] = ratio;
  }
  for (int k = 0; k < LS_NS; ++k) {
    double v = acc[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) sh[k][wave] = v;
  }
  __syncthreads();
  if (threadIdx.x < LS_NS)
    partial[(int64_t)blockIdx.x * LS_NS + threadIdx.x] =
        (sh[threadIdx.x][0] + sh[threadIdx.x][1]) + (sh[threadIdx.x][2] + sh[threadIdx.x][3]);
}

// one workgroup per sum: strided per-thread sums over the block partials, then a shared-memory tree (fixed order)
__global__ __launch_bounds__(256) void ma_trpo_ls_finish_kernel(const double* __restrict__ partial, int nblocks,
                                                                double* __restrict__ sums_out) {
  __shared__ double shp[256];
  const int k = blockIdx.x;
  double s = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += 256) s += partial[(int64_t)b * LS_NS + k];
  shp[threadIdx.x] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) shp[threadIdx.x] += shp[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) sums_out[k] = shp[0];
}
}  // namespace

extern "C" int spo_ma_trpo_linesearch_sums(const float* mean, const float* log_std, float std_x_coef, float std_y_coef,
                                           const float* act, const float* old_logp, const float* adv, const float* cost_adv,
                                           const float* factor, const float* mu_old, const float* std_old, int64_t rows,
                                           int act_dim, double* sums4_out, float* ratio_out_or_null, double* partial_ws,
                                           void* stream) {
  SPO_REQUIRE(mean && log_std && act && old_logp && adv && cost_adv && factor && mu_old && std_old && sums4_out && partial_ws,
              "ma_trpo_linesearch_sums: null pointer");
  if (act_dim < 1 || act_dim > SPO_MAX_ACT)
    return spo::fail(-2, "ma_trpo_linesearch_sums: act_dim %d outside [1,%d]", act_dim, SPO_MAX_ACT);
  SPO_REQUIRE(rows >= 1, "ma_trpo_linesearch_sums: rows must be >= 1");
  hipStream_t st = (hipStream_t)stream;
  const int64_t g = (rows + 255) / 256;
  const int gr = (int)(g > LS_MAX_BLOCKS ? LS_MAX_BLOCKS : g);
  hipLaunchKernelGGL(ma_trpo_ls_kernel, dim3(gr), dim3(256), 0, st, mean, log_std, std_x_coef, std_y_coef, act, old_logp, adv,
                     cost_adv, factor, mu_old, std_old, ratio_out_or_null, partial_ws, rows, act_dim);
  hipLaunchKernelGGL(ma_trpo_ls_finish_kernel, dim3(LS_NS), dim3(256), 0, st, partial_ws, gr, sums4_out);
  SPO_LAUNCH_CHECK("spo_ma_trpo_linesearch_sums");
  return 0;
}

// ---------------------------------------------------------------- MACPO conjugate gradient: the vector step on the device
// Reference safepo/multi_agent/macpo.py:168-185.  The host-driven loop ran ~8 torch launches per iteration around the
// Fisher-vector product and read `rdotr < residual_tol` on the host every iteration -- a queue drain before the next product's
// ~20 launches can be issued, and under data parallelism a cross-rank stall.  Here x, r, p and {rdotr, done} live on the device:
//     init:    x = 0, r = p = b, rdotr = b.b
//     update:  alpha = rdotr / (p.avp + 1e-8);  x += alpha p;  r -= alpha avp;  new = r.r;  p = r + (new / rdotr) p;  rdotr = new;
//              done = new < residual_tol, and a set flag turns every later update into a no-op (the reference's `break`)
// so a solve is enqueued as a whole.  Dot products accumulate in fp64 and round once to fp32; the scalar recurrences are fp32 in
// the reference's order.  Fixed-order reductions: wave shuffle tree -> the workgroup's waves in order -> per-block partials in
// order.  Up to CG_PER_BLOCK elements one workgroup does the whole update in ONE launch; beyond, p.avp is a launch of its own and
// the step launch forms alpha from its partials in every workgroup, updates x and r, and the LAST workgroup to arrive (an
// integer arrival counter; no float atomics) sums the r.r partials and writes p -- two launches for any n, no grid barrier.
// ws: double[SPO_MA_CG_WS_DOUBLES] = {p.avp partials[256], r.r partials[256], arrival counter}; state: float[4] =
// {rdotr, done, last alpha, last beta}.
namespace {
constexpr int CG_THREADS = 1024, CG_PER_BLOCK = 16384, CG_MAX_BLOCKS = 256;
static_assert(2 * CG_MAX_BLOCKS + 1 <= SPO_MA_CG_WS_DOUBLES, "workspace layout");

int cg_blocks(int64_t n) {
  const int64_t g = (n + CG_PER_BLOCK - 1) / CG_PER_BLOCK;
  return (int)(g > CG_MAX_BLOCKS ? CG_MAX_BLOCKS : g);
}

// sum over the workgroup, the same value in every thread; sh: double[CG_THREADS / 64]
__device__ __forceinline__ double cg_block_sum(double v, double* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();                                   // a previous sum's readers are through with sh
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < CG_THREADS / 64; ++w) s += sh[w];
  return s;
}

// sum of nparts (<= CG_MAX_BLOCKS) block partials written by OTHER workgroups (of this launch or the one before)
__device__ __forceinline__ double cg_sum_partials(const double* partial, int nparts, double* sh) {
  const volatile double* vp = partial;
  return cg_block_sum((int)threadIdx.x < nparts ? vp[threadIdx.x] : 0.0, sh);
}

// true in every thread of the last workgroup to arrive; its later reads see what the other workgroups wrote before arriving
__device__ __forceinline__ bool cg_arrive_last(unsigned* counter, int* flag_sh) {
  __threadfence();                                   // every thread's stores are visible device-wide ...
  __syncthreads();                                   // ... before the workgroup announces itself
  if (threadIdx.x == 0) *flag_sh = atomicAdd(counter, 1u) == gridDim.x - 1;
  __syncthreads();
  const bool last = *flag_sh != 0;
  if (last) __threadfence();
  return last;
}

__global__ __launch_bounds__(CG_THREADS) void ma_cg_init_kernel(const float* __restrict__ b, float* __restrict__ x,
                                                                float* __restrict__ r, float* __restrict__ p,
                                                                float* state, double* ws, int64_t n) {
  __shared__ double sh[CG_THREADS / 64];
  __shared__ int flag;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * CG_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * CG_THREADS) {
    const float v = b[i];
    x[i] = 0.f; r[i] = v; p[i] = v;
    acc += (double)v * (double)v;
  }
  double rr = cg_block_sum(acc, sh);
  unsigned* counter = reinterpret_cast<unsigned*>(ws + 2 * CG_MAX_BLOCKS);
  if (gridDim.x > 1) {
    if (threadIdx.x == 0) ws[CG_MAX_BLOCKS + blockIdx.x] = rr;
    if (!cg_arrive_last(counter, &flag)) return;
    rr = cg_sum_partials(ws + CG_MAX_BLOCKS, (int)gridDim.x, sh);
  }
  if (threadIdx.x == 0) {
    state[0] = (float)rr; state[1] = 0.f; state[2] = 0.f; state[3] = 0.f;
    *counter = 0u;
  }
}

__global__ __launch_bounds__(CG_THREADS) void ma_cg_dot_kernel(const float* __restrict__ p, const float* __restrict__ avp,
                                                               const float* __restrict__ state, double* __restrict__ ws, int64_t n) {
  __shared__ double sh[CG_THREADS / 64];
  if (state[1] != 0.f) return;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * CG_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * CG_THREADS)
    acc += (double)p[i] * (double)avp[i];
  const double s = cg_block_sum(acc, sh);
  if (threadIdx.x == 0) ws[blockIdx.x] = s;
}

__global__ __launch_bounds__(CG_THREADS) void ma_cg_step_kernel(const float* __restrict__ avp, float* x, float* r, float* p,
                                                                float* state, double* ws, int64_t n, float residual_tol) {
  __shared__ double sh[CG_THREADS / 64];
  __shared__ int flag;
  // the flag and rdotr change only in the tail below, which runs after every workgroup of this launch has read them
  if (state[1] != 0.f) return;
  const float rdotr = state[0];
  const int64_t first = (int64_t)blockIdx.x * CG_THREADS + threadIdx.x, stride = (int64_t)gridDim.x * CG_THREADS;
  double pap;
  if (gridDim.x == 1) {
    double acc = 0.0;
    for (int64_t i = first; i < n; i += stride) acc += (double)p[i] * (double)avp[i];
    pap = cg_block_sum(acc, sh);
  } else {
    pap = cg_sum_partials(ws, (int)gridDim.x, sh);
  }
  const float alpha = rdotr / ((float)pap + 1e-8f);
  double acc = 0.0;
  for (int64_t i = first; i < n; i += stride) {
    x[i] = x[i] + alpha * p[i];
    const float ri = r[i] - alpha * avp[i];
    r[i] = ri;
    acc += (double)ri * (double)ri;
  }
  double rr = cg_block_sum(acc, sh);
  unsigned* counter = reinterpret_cast<unsigned*>(ws + 2 * CG_MAX_BLOCKS);
  if (gridDim.x > 1) {
    if (threadIdx.x == 0) ws[CG_MAX_BLOCKS + blockIdx.x] = rr;
    if (!cg_arrive_last(counter, &flag)) return;
    rr = cg_sum_partials(ws + CG_MAX_BLOCKS, (int)gridDim.x, sh);
  }
  const float new_rdotr = (float)rr;
  const float beta = new_rdotr / rdotr;
  const volatile float* rv = r;                      // rows of r written by the other workgroups of this launch
  for (int64_t i = threadIdx.x; i < n; i += CG_THREADS) p[i] = rv[i] + beta * p[i];
  if (threadIdx.x == 0) {
    state[0] = new_rdotr; state[1] = new_rdotr < residual_tol ? 1.f : 0.f; state[2] = alpha; state[3] = beta;
    if (gridDim.x > 1) *counter = 0u;
  }
}
}  // namespace

extern "C" int spo_ma_cg_init(const float* b, float* x, float* r, float* p, float* state4, double* ws, int64_t n, void* stream) {
  SPO_REQUIRE(b && x && r && p && state4 && ws, "ma_cg_init: null pointer");
  SPO_REQUIRE(n >= 1, "ma_cg_init: n must be >= 1");
  hipStream_t st = (hipStream_t)stream;
  if (int rc = spo::hip_check(hipMemsetAsync(ws + 2 * CG_MAX_BLOCKS, 0, sizeof(double), st), "ma_cg_init: counter reset")) return rc;
  hipLaunchKernelGGL(ma_cg_init_kernel, dim3(cg_blocks(n)), dim3(CG_THREADS), 0, st, b, x, r, p, state4, ws, n);
  SPO_LAUNCH_CHECK("spo_ma_cg_init");
  return 0;
}

extern "C" int spo_ma_cg_update(const float* avp, float* x, float* r, float* p, float* state4, double* ws, int64_t n,
                                float residual_tol, void* stream) {
  SPO_REQUIRE(avp && x && r && p && state4 && ws, "ma_cg_update: null pointer");
  SPO_REQUIRE(n >= 1, "ma_cg_update: n must be >= 1");
  hipStream_t st = (hipStream_t)stream;
  const int g = cg_blocks(n);
  if (g > 1) hipLaunchKernelGGL(ma_cg_dot_kernel, dim3(g), dim3(CG_THREADS), 0, st, p, avp, state4, ws, n);
  hipLaunchKernelGGL(ma_cg_step_kernel, dim3(g), dim3(CG_THREADS), 0, st, avp, x, r, p, state4, ws, n, residual_tol);
  SPO_LAUNCH_CHECK("spo_ma_cg_update");
  return 0;
}
