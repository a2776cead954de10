// MACPO line search: the terms of one row of one candidate, shared by the row pass over a materialised mean
// (spo_ma_trpo_linesearch_sums, multi_agent.hip) and the fused candidate evaluation (spo_ma_ls_eval, ma_ls_eval.hip).
// Reference safepo/multi_agent/macpo.py:329-366 up to the accept test; every kernel keeps its own loops and storage, the
// arithmetic and its order are here.
#pragma once
#include "common.h"

namespace spo {

constexpr float MA_LOG_SQRT_2PI_F = 0.91893853320467274178f;
constexpr int MA_LS_NS = 4;      // {sum ratio*factor*adv, sum ratio*factor*cost_adv, sum KL_row, sum ratio}

// per action dimension, the same for every row: std = yc * sigmoid(log_std / xc), std_old^2, log std_old - log std
__device__ __forceinline__ void ma_ls_dim_consts(float log_std, float std_old, float xc, float yc, float& sd, float& so2, float& dlog) {
  sd = yc / (1.f + expf(-log_std / xc));
  so2 = std_old * std_old;
  dlog = logf(std_old) - logf(sd);
}

// one action dimension of one row: ratio *= exp(logp_d - old_logp_d) with logp_d exactly as ma_logp_kernel (ma_net.hip) forms it
// (torch.exp per dimension, then torch.prod), kl += the dimension's term of kl_divergence (macpo.py:153-166, as written)
__device__ __forceinline__ void ma_ls_dim_term(float mu, float act, float old_logp, float mu_old, float sd, float so2, float dlog,
                                               float& ratio, float& kl) {
  const float d = act - mu;
  const float lp = -(d * d) / (2.f * sd * sd) - logf(sd) - MA_LOG_SQRT_2PI_F;
  ratio *= expf(lp - old_logp);
  const float dm = mu_old - mu;
  kl += dlog + (so2 + dm * dm) / (1e-8f + 2.f * sd * sd) - 0.5f;
}

// one action dimension's log-probability as ma_ls_dim_term forms it, and d = act - mu: the row terms of the surrogate loss and of
// its cotangent (spo_ma_trpo_grads, ma_trpo_grads.hip)
__device__ __forceinline__ float ma_logp_dim(float mu, float act, float sd, float& d) {
  d = act - mu;
  return -(d * d) / (2.f * sd * sd) - logf(sd) - MA_LOG_SQRT_2PI_F;
}

// the row's four terms, rounded to fp32 as the reference's products are, added in fp64
__device__ __forceinline__ void ma_ls_row_add(float ratio, float kl, float factor, float adv, float cost_adv, double (&acc)[MA_LS_NS]) {
  const float w = ratio * factor;
  acc[0] += (double)(w * adv);
  acc[1] += (double)(w * cost_adv);
  acc[2] += (double)kl;
  acc[3] += (double)ratio;
}

}  // namespace spo
