// Internal interface of the row-split persistent update kernel (update_rs.hip), called from update.hip's entry points.
#pragma once
#include <cstddef>
#include <cstdint>
#include "../../include/safepo_hip.h"

namespace spo {
// n_nets 3: one learning iteration of the PPO-Lagrangian step (clipped surrogate); 2: the critic fit (act / logp_old / adv unused).
// prof: optional device [3][12] u64 cycle accumulators (instrumented instantiation, obs_dim in (32, 64], batch <= 64).
int rs_update_launch(float* theta, float* adam_m, float* adam_v, int64_t adam_step_host, const float* obs, const float* act,
                     const float* logp_old, const float* target_r, const float* target_c, const float* adv, const int32_t* perm,
                     int64_t M, const spo_ppo_cfg* cfg_host, int n_nets, float* stale_sq_io, float* losses_out, void* sync_ws,
                     unsigned long long* prof, void* stream);
// one rank of a data-parallel job (update.hip: spo_ppo_lag_update_iter_dp with SPO_XR_FORM_ROW_SPLIT); RSX_BYTES of every rank's
// exchange region at offset rsx_off belong to this form: [parity 2][row group 2][network 3][source rank 8][word 16][lane 256] x 16 B
constexpr size_t RSX_BYTES = (size_t)2 * 2 * 3 * 8 * 16 * 4096;
int rs_update_launch_dp(float* theta, float* adam_m, float* adam_v, int64_t adam_step_host, const float* obs, const float* act,
                        const float* logp_old, const float* target_r, const float* target_c, const float* adv, const int32_t* perm,
                        int64_t M, const spo_ppo_cfg* cfg_host, float* losses_out, void* sync_ws, int rank, int world,
                        void* const* regions, uint32_t step0, size_t rsx_off, void* stream);
// {minibatch steps run, steps redone after a late clip verdict} of the row-split kernel since the last reset
int rs_counters(unsigned long long* out2_host, int reset);
// row groups (2 or 4) the one-GPU launch above runs for this shape (SPO_RS_ROWS, read once per process)
int rs_row_groups(int obs_dim, int batch);
// scratch blocks of the replica-batched launch (spo_ppo_lag_update_iter_multi), freed by spo_update_scratch_release
int rs_multi_scratch_release(int dev, void* stream_or_null, int all);
// Block map of the replica-batched launches (update_rs.hip: ppo_update_rs_multi_kernel; update.hip: ppo_update_multi_kernel).
// Workgroups are dealt to the XCDs round-robin by block index (a placement hint: speed only), so block b carries XCD label b & 7;
// of the blocks with one label, `wgs` consecutive ones serve one replica: replica r sits on label r & 7, replicas r, r + 8, ...
// share an XCD and its L2.  Host and device share this function (spo_rs_multi_block_map and its kin).  False: the block has no work.
// `wgs`: workgroups per replica -- 6 for the PPO-Lagrangian step (at most SPO_RS_MAX_REPLICAS / 8 = 4 replicas per XCD: 24 workgroups
// of one CU each on the XCD's 32 CUs), 8 for the critic fit (SPO_RS_CRITIC_MAX_REPLICAS / 8 = 3 per XCD, again 24), and the number of
// networks (3, or 1 actor alone) for the four-wave step of spo_update_iter_ex_multi (at most 4 replicas: 12 workgroups per XCD).
__host__ __device__ inline bool rs_multi_map(int block, int n_replicas, int wgs, int* replica, int* wg) {
  const int x = block & 7, k = block >> 3;
  *replica = 8 * (k / wgs) + x;
  *wg = k % wgs;
  return *replica < n_replicas;
}
inline int rs_multi_grid(int n_replicas, int wgs) { return 8 * wgs * ((n_replicas + 7) / 8); }
}  // namespace spo
