// The table-driven (seed-batched) form of spo_wide_clip_adam_dev_log's three launches, for the row-group KL-penalty step of
// csrc/mlp_rows.hip (spo_wide_rows_ex_step_multi).  The kernels and their argument structs stay in csrc/wide.hip's anonymous
// namespace; a caller in another file holds its runs' entries as opaque bytes behind its own table:
//   wide_opt_entry_bytes()  size of one run's entry (a multiple of 8: lay the entries out at an 8-byte aligned address);
//   wide_opt_fill()         one run's entry from what spo_wide_clip_adam_dev_log takes -- the checks and the argument filling of
//                           that entry point (wide_fill_opt, the one place both forms get their kernel arguments from); no HIP call;
//   wide_opt_launch_multi() prep (over [norm_begin, n_params) when norm_begin != 0) -> coefficient (one wave per run) -> Adam, run r
//                           on blockIdx.y == r with the stand-alone launch's blockIdx.x / gridDim.x; an entry of zero bytes is an
//                           inactive run, whose blocks return after reading its `active` word.
#pragma once
#include <cstddef>
#include <cstdint>
#include <hip/hip_runtime.h>
#include "../../include/safepo_hip.h"

namespace spo {
size_t wide_opt_entry_bytes();
int wide_opt_fill(const char* entry, void* entry_out, float* theta, float* grad, float* adam_m, float* adam_v, int64_t n_params,
                  int64_t reward_critic_end, int64_t cost_critic_end, int64_t actor_begin, const spo_ppo_cfg* cfg, double* pow4_dev,
                  int64_t adam_begin, int64_t adam_end, int64_t norm_begin, int scale_rest, float* losses3_inout, float* scalars4_out,
                  double* partial_ws, int partial_capacity, float* loss_log_dev, const float* log_src_dev, int64_t* cursor_dev,
                  int64_t cursor_step);
void wide_opt_launch_multi(const void* entries_dev, int n_replicas, int64_t n_params, int64_t norm_begin, hipStream_t stream);
}  // namespace spo
