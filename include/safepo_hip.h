/*
 * safepo_hip.h -- C ABI of libsafepo_hip.so (gfx950 / MI355X).
 *
 * The reference (PKU-Alignment/Safe-Policy-Optimization) has NO native layer: the path
 * this library replaces is Python.  Each entry point below names the
 * reference Python function (file:line relative to /root/reference) whose arithmetic it
 * replaces; the Python host mirror (safe-policy-optimization_amd/safepo) binds them with ctypes.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in _host;
 *   - no allocation, no ownership transfer, no implicit synchronisation; work is enqueued on
 *     `stream` (a hipStream_t passed as void*; NULL = default stream);
 *   - return value: 0 ok, <0 argument error (see spo_last_error()), >0 a hipError_t;
 *   - re-entrant per stream; one host thread per GPU.
 *
 * Dense on-policy buffer layout (replaces the list of per-env dicts,
 * safepo/common/buffer.py:53-73): scalars are [num_envs, T] env-major (flat row = env*T + t,
 * the order VectorizedOnPolicyBuffer.get() concatenates in, buffer.py:149-153), obs
 * [num_envs, T, obs_dim], act [num_envs, T, act_dim]; path ends are a u8 mask seg_end[N,T]
 * with the bootstrap values of finish_path() in boot_r/boot_c[N,T].
 *
 * Flat parameter vector `theta` (fp32): policy.parameters() order of ActorVCritic
 * (safepo/common/model.py:131-135): reward_critic {W1[H,D],b1,W2[H,H],b2,W3[1,H],b3},
 * cost_critic {same}, actor {log_std[A], W1[H,D],b1,W2[H,H],b2,W3[A,H],b3}; nn.Linear
 * row-major [out,in].  H = 64 (default_cfg hidden_sizes, ppo_lag.py:45-52).
 */
#ifndef SAFEPO_HIP_H
#define SAFEPO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPO_ABI_VERSION 2        /* 2 (round 6): pow4_dev of spo_wide_clip_adam_dev(_log) is double[6], a negative learning-rate entry
                                 * means "the cfg's"; spo_update_rs_supported; the row-split form behind spo_ppo_lag_update_iter */
#define SPO_HIDDEN 64          /* hidden width the MLP kernels are specialised for          */
#define SPO_MAX_ACT 16         /* act_dim <= 16 (one MFMA output tile; LDS-resident kernels) */
#define SPO_MAX_OBS 128        /* obs_dim <= 128 (LDS-resident kernels; CPO full-batch kernels: 64) */
#define SPO_WIDE_MAX_ACT 64    /* act_dim limit of the wide-network path (any obs_dim / hidden_sizes): its actor-side loss kernels
                                * give a batch row pow2ceil(act_dim) lanes of ONE 64-lane wavefront and sum over the action
                                * dimension with segmented shuffles; a wider action vector would need a row spread over several
                                * wavefronts.  The widest action space of the reference's task sets is 17 (Humanoid). */
#define SPO_GAE_PARTIAL_STRIDE 16 /* doubles per block written by spo_gae_fused: 4 waves x 4 */

int spo_abi_version(void);
const char* spo_last_error(void);

/* ---- a-5: VectorizedOnPolicyBuffer.finish_path -> calculate_adv_and_value_targets ->
 *      discount_cumsum (safepo/common/buffer.py:97-140,191-201,167-188), for ALL paths of
 *      ALL envs and for reward and cost in one launch.
 * delta in fp32 (three separately rounded ops, gamma rounded to fp32), segmented backward
 * scan in fp64 with discount gamma*lam formed in double, results rounded to fp32.
 * Steps after the last seg_end of a row (unfinished path) get adv = target = 0.
 * boot_r == boot_c == NULL selects the FOLDED form: `reward` / `cost` are then the arrays written by
 * spo_boundary_step_fold (gamma * bootstrap already added at path ends); same results, no bootstrap loads.
 * partials: [spo_gae_num_blocks(N,T)][SPO_GAE_PARTIAL_STRIDE] doubles: one row {sum adv_r, sum adv_r^2, sum adv_c,
 * count} per wave of each workgroup (no block-level combine inside the scan; spo_adv_reduce adds the rows). */
int spo_gae_num_blocks(int64_t num_envs, int64_t T);
int spo_gae_fused(const float* reward, const float* cost, const float* value_r, const float* value_c,
                  const uint8_t* seg_end, const float* boot_r, const float* boot_c,
                  float* adv_r, float* adv_c, float* target_r, float* target_c,
                  double* partials, int64_t num_envs, int64_t T,
                  double gamma, double lam, double lam_c, void* stream);

/* Debug/bench knob: 0 = automatic, 1 = eager bootstrap loads (latency-optimised, cache-resident
 * buffers), 2 = predicated bootstrap loads (fewest bytes, HBM-streaming buffers). */
int spo_debug_gae_variant(int v);
/* Measurement aid (bench.py `roofline`): spo_gae_fused `reps` times on `stream`, every dispatch carrying its own start /
 * stop events, so durations_us_host[i] (host array of `reps` floats) is the execution time of dispatch i as the dispatch
 * packet's own timestamps record it -- the per-dispatch figure rocprofv3 --kernel-trace reports.  Synchronises `stream`. */
int spo_gae_fused_timed(const float* reward, const float* cost, const float* value_r, const float* value_c,
                        const uint8_t* seg_end, const float* boot_r, const float* boot_c,
                        float* adv_r, float* adv_c, float* target_r, float* target_c,
                        double* partials, int64_t num_envs, int64_t T,
                        double gamma, double lam, double lam_c, int reps, float* durations_us_host, void* stream);

/* ---- a-6: statistics of VectorizedOnPolicyBuffer.get() (buffer.py:154-160).
 * spo_adv_reduce: partials -> sums[4] = {sum adv_r, sum adv_r^2, sum adv_c, count} (fixed order,
 * deterministic).  Multi-GPU: all-reduce(sum) sums[] between the two calls.
 * spo_adv_apply: adv_r <- (adv_r-mean)/(std_unbiased+1e-8) if standardize_r; adv_c <- adv_c-mean_c
 * if standardize_c; a-8 (ppo_lag.py:280-281): adv_mix = (adv_r - lambda*adv_c)/(lambda+1) when
 * adv_mix != NULL.  stats_out (optional, 3 floats): mean_r, std_r, mean_c. */
int spo_adv_reduce(const double* partials, int num_blocks, double* sums, void* stream);
int spo_adv_apply(float* adv_r, float* adv_c, float* adv_mix, const double* sums, int64_t count,
                  double lagrangian_multiplier, int standardize_r, int standardize_c,
                  float* stats_out, void* stream);

/* ---- a-1/a-3: ActorVCritic.step (safepo/common/model.py:149-170) + buffer.store
 * (buffer.py:84-95) for step t of every env.  act = mean + exp(log_std)*eps (rsample with the
 * noise supplied; eps == NULL -> deterministic, act = mean).  Outputs act/logp/v_r/v_c [N,...];
 * when buf_* are non-NULL the same values (and obs) are also written to slot t of the dense
 * buffer. */
int spo_policy_step(const float* theta, const float* obs, const float* eps,
                    float* act, float* logp, float* v_r, float* v_c,
                    float* buf_obs, float* buf_act, float* buf_logp, float* buf_v_r, float* buf_v_c,
                    int64_t num_envs, int64_t T, int64_t t, int obs_dim, int act_dim, void* stream);

/* ---- a-2: observation normalisation of SafeNormalizeObservation (safepo/common/wrappers.py:42-49 ->
 * gymnasium NormalizeObservation / RunningMeanStd, third-party, restated from its documented algorithm:
 * PARITY UNPINNED).  rms_state = double[2*obs_dim+1] = mean[D], var[D], count (init 0, 1, 1e-4).
 * update != 0: merge this batch (mean, biased var over num_envs) into the running statistics first;
 * then obs <- (obs - mean) / sqrt(var + 1e-8), in place. */
int spo_obs_normalize(float* obs, double* rms_state, int64_t num_envs, int obs_dim, int update, void* stream);

/* a-1 + a-2 fused (north_star: "fused obs-normalise + MLP forward"): spo_policy_step on RAW observations with the
 * SafeNormalizeObservation wrapper's arithmetic (wrappers.py:42-49 -> gymnasium NormalizeObservation / RunningMeanStd) folded
 * in.  update != 0: the batch is first merged into rms_state (mean[D], var[D], count; fp64; parallel-variance merge).  Then
 * every row is read ONCE, normalised in registers as (float)(((double)x - mean) / sqrt(var + 1e-8)), fed to the three
 * networks, stored to the buffer slot and written back to obs_inout (the wrapper hands the normalised observation on). */
int spo_policy_step_norm(const float* theta, float* obs_inout, double* rms_state, int update, const float* eps,
                         float* act, float* logp, float* v_r, float* v_c,
                         float* buf_obs, float* buf_act, float* buf_logp, float* buf_v_r, float* buf_v_c,
                         int64_t num_envs, int64_t T, int64_t t, int obs_dim, int act_dim, void* stream);

/* critics only (bootstrap values of ppo_lag.py:201-215): v_r, v_c for `rows` observations. */
int spo_values(const float* theta, const float* obs, float* v_r, float* v_c,
               int64_t rows, int obs_dim, int act_dim, void* stream);

/* ---- a-4: path-boundary logic of the collect loop (ppo_lag.py:198-234) for step t:
 * seg_end = epoch_end | terminated | truncated; boot = 0 if terminated, else value(next obs) at
 * epoch end, overridden by value(final obs) if truncated.  Also stores reward/cost of the step,
 * accumulates ep_ret/ep_cost/ep_len (ppo_lag.py:168-170) and appends one record
 * {t*num_envs + env, ep_ret, ep_cost, ep_len} (4 doubles) per finished episode to `events`, in
 * env order (the order of the reference's Python loop); events_count is a device int advanced
 * by the single block that runs this kernel. */
int spo_boundary_step(const float* reward, const float* cost, const float* terminated, const float* truncated,
                      const float* v_next_r, const float* v_next_c, const float* v_final_r, const float* v_final_c,
                      float* buf_reward, float* buf_cost, uint8_t* seg_end, float* boot_r, float* boot_c,
                      double* ep_ret, double* ep_cost, double* ep_len, double* events, int* events_count,
                      int events_capacity, int64_t num_envs, int64_t T, int64_t t, int epoch_end, void* stream);

/* The same step, additionally writing the two arrays spo_gae_fused reads in its FOLDED form (boot_r == boot_c == NULL
 * there): fold_reward[env,t] = fl(reward + fl((float)gamma * boot_r)) at a path end and the plain reward elsewhere (same
 * for cost) -- the first two of the three fp32 operations of delta_t = r_t + gamma*v_{t+1} - v_t (buffer.py:198) applied
 * to the value finish_path would append (buffer.py:118-125).  The scan then needs no bootstrap loads: exactly the 33
 * algorithmic bytes per (env, step), no second memory round trip, results bit-identical to the unfolded form. */
int spo_boundary_step_fold(const float* reward, const float* cost, const float* terminated, const float* truncated,
                           const float* v_next_r, const float* v_next_c, const float* v_final_r, const float* v_final_c,
                           float* buf_reward, float* buf_cost, uint8_t* seg_end, float* boot_r, float* boot_c,
                           double* ep_ret, double* ep_cost, double* ep_len, double* events, int* events_count,
                           int events_capacity, int64_t num_envs, int64_t T, int64_t t, int epoch_end,
                           float* fold_reward, float* fold_cost, double gamma, void* stream);

/* The same step on num_envs / 256 workgroups instead of one (the one-block kernel is a 24 us latency chain at 4 096 envs).  The
 * running event count lives in events_prefix (int[T + 1], events_prefix[0] = 0 at the start of an epoch): the kernel of step t
 * reads events_prefix[t], appends this step's finished episodes in env order and writes events_prefix[t + 1]; after the epoch
 * events_prefix[T] records are valid.  fold_reward / fold_cost may both be NULL.  Everything else as spo_boundary_step_fold;
 * results (buffers, masks, event log) are identical. */
int spo_boundary_step_fold_mb(const float* reward, const float* cost, const float* terminated, const float* truncated,
                              const float* v_next_r, const float* v_next_c, const float* v_final_r, const float* v_final_c,
                              float* buf_reward, float* buf_cost, uint8_t* seg_end, float* boot_r, float* boot_c,
                              double* ep_ret, double* ep_cost, double* ep_len, double* events, int* events_prefix,
                              int events_capacity, int64_t num_envs, int64_t T, int64_t t, int epoch_end,
                              float* fold_reward, float* fold_cost, double gamma, void* stream);

/* spo_values(theta, final_obs) -> (v_final_r, v_final_c) and spo_boundary_step_fold_mb with those values, in ONE launch (the
 * post-step half of a collect step, ppo_lag.py:198-234): the bootstrap values of truncated envs go from the critics' accumulators
 * to the boundary logic through LDS.  v_final_r / v_final_c are still written.  Same results as the two calls (which it makes
 * itself outside the side-by-side kernel's envelope: obs_dim > 64 or more than 8 192 envs). */
int spo_values_boundary_step_fold(const float* theta, const float* final_obs, float* v_final_r, float* v_final_c,
                                  int obs_dim, int act_dim, const float* reward, const float* cost,
                                  const float* terminated, const float* truncated, const float* v_next_r,
                                  const float* v_next_c, float* buf_reward, float* buf_cost, uint8_t* seg_end,
                                  float* boot_r, float* boot_c, double* ep_ret, double* ep_cost, double* ep_len,
                                  double* events, int* events_prefix, int events_capacity, int64_t num_envs,
                                  int64_t T, int64_t t, int epoch_end, float* fold_reward, float* fold_cost,
                                  double gamma, void* stream);

/* ---- a-9/a-10: one learning iteration of the PPO-Lagrangian update (ppo_lag.py:297-336):
 * for each consecutive chunk of `batch` indices of perm[M] (last partial chunk kept): gather,
 * 3x MLP fwd, loss_r/loss_c (MSE + 0.001*L2 if use_critic_norm), clipped surrogate, backward,
 * joint clip_grad_norm_(max_grad_norm, eps 1e-6), 3x Adam (betas .9/.999, eps 1e-8).
 * Persistent kernel, 3 workgroups (one per network) for the whole iteration; weights in LDS,
 * Adam moments in registers for the launch (loaded from / stored to adam_m, adam_v).
 * adam_step_host: number of optimiser steps already taken (bias correction continues from it).
 * losses_out: [num_minibatches][3] = loss_r, loss_c, loss_pi per minibatch (ppo_lag.py:330-336).
 * sync_ws: >= 72 bytes of device scratch, zero before first use.  Bytes 0..63 are exchange slots, zeroed by every
 * call; the int at byte 64 is a STICKY error word the kernels only ever set (1 = inter-workgroup exchange timed out,
 * 2 = a peer rank never answered the in-kernel gradient exchange) -- the caller reads and clears it.                */
typedef struct {
  int obs_dim, act_dim, batch;
  int use_critic_norm;          /* config.get("use_critic_norm", True)                        */
  int use_value_coefficient;    /* total = loss_pi + 2*loss_r + loss_c                        */
  float clip;                   /* 0.2                                                         */
  float max_grad_norm;          /* 40.0                                                        */
  float lr_actor, lr_critic;    /* 3e-4 * LinearLR factor, 3e-4                                */
  float beta1, beta2, adam_eps; /* 0.9, 0.999, 1e-8                                            */
  float l2_coef;                /* 0.001                                                       */
} spo_ppo_cfg;

int spo_ppo_lag_update_iter(float* theta, float* adam_m, float* adam_v, int64_t adam_step_host,
                            const float* obs, const float* act, const float* logp_old,
                            const float* target_r, const float* target_c, const float* adv,
                            const int32_t* perm, int64_t M, const spo_ppo_cfg* cfg_host,
                            float* losses_out, void* sync_ws, void* stream);

/* The main + helper form of the persistent update keeps one ~790 KB scratch block (clip backups, norm granules) per
 * (device, stream handle) pair, allocated at that pair's first launch (never under stream capture: launch once outside the
 * capture first) and kept; at most 256 pairs per process.  A process that keeps creating and destroying streams releases a
 * stream's block before destroying it: returns the number of blocks freed (>= 0) for (current device, stream), or for every
 * stream of the current device when all != 0.  hipFree synchronises the device -- not for the hot path. */
int spo_update_scratch_release(void* stream_or_null, int all);

/* Round 6: the ROW-SPLIT form of the persistent update (csrc/update_rs.hip) -- the rows of every minibatch divided over R
 * co-XCD workgroups per network (R = 2 up to 64 rows, 4 up to 128), partial weight gradients all-reduced in one hand-off through
 * the XCD's L2, replicated Adam.  spo_ppo_lag_update_iter (n_nets 3; ppo_lag.py:297-336) and spo_critic_fit_iter (n_nets 2;
 * cpo.py:534-571) run on it where this returns 1 (obs_dim <= 64, act_dim <= 16, batch <= 64 / 128) unless SPO_UPDATE_FORM=2
 * (the main + helper form) or 0 (the four-wave form) is set in the environment.  Same arguments, same results to rounding. */
int spo_update_rs_supported(int obs_dim, int act_dim, int batch, int n_nets);

/* The row-split form for observations of 65 .. 128 values (a KIN = 128 instantiation of the same kernel: the Car / Racecar / Doggo /
 * Ant navigation tasks).  Layer 1's optimiser state does not fit a 256-register wave the way it is held up to 64 inputs, so the
 * x^T operands of its weight gradient pass through the registers in two halves, its parameters stay in LDS until they are used, and
 * its Adam step runs behind the joint norm with the clip coefficient in hand (no speculation, no backups, no redo).  Returns 1
 * exactly for 65 <= obs_dim <= 128, 1 <= act_dim <= 16, 1 <= batch <= 64 and n_nets == 3: spo_ppo_lag_update_iter then runs on it
 * unless SPO_RS_OBS128=0 (read at every launch: the four-wave kernel, as before) or SPO_UPDATE_FORM < 3 is set.  n_nets == 2 (the
 * critic fit, four row groups) returns 0: that instantiation was measured slower than the forms it would replace and is not built.
 * A separate question from spo_update_rs_supported, which stays 0 above 64: it also keys the data-parallel routing, and the
 * data-parallel row-split form has no KIN = 128 instantiation.  In spo_debug_update_counters the form's steps count as row-split
 * steps; nothing is redone in it, the second counter counts its steps whose joint clip was active. */
int spo_update_rs128_supported(int obs_dim, int act_dim, int batch, int n_nets);

/* Staged minibatch inputs of the row-split PPO-Lagrangian step (two row groups, obs_dim <= 64, one GPU).  What a step reads of the
 * buffer depends only on perm, the buffer and the shapes, so spo_ppo_lag_update_iter gathers it in a full-machine pre-pass on the
 * caller's stream, once per launch, into one record per minibatch step -- x[64][KIN] with pad features zero, the same transposed,
 * act[64][16], logp_old / adv / target_r / target_c[64]; KIN = 16 / 32 / 64, columns past `batch` zero -- and the persistent kernel
 * reads records instead of gathering in its step.  Same bits.  The block belongs to the (device, stream) pair like the exchange
 * scratch, grows on demand (never inside a capture: such a launch gathers in the kernel unless the block is already large
 * enough) and is freed by spo_update_scratch_release.  Environment, read at every launch: SPO_RS_STAGE=0 turns it off,
 * SPO_RS_STAGE_MAX_MB (default 1024) bounds the block -- a launch that would need more, or 2 GiB or more, gathers in the kernel,
 * and so does the one-batch A/B form of the 33-64-observation kernel (SPO_RS_L1_PIPE=0).
 * spo_rs_stage_bytes: the block's size for a launch of M samples ((M + batch - 1) / batch records), 0 where the staged form does
 * not apply (obs_dim > 64, batch > 64 -- the critic fit's 128-row minibatches --, SPO_RS_ROWS=16).  Needs no GPU. */
int64_t spo_rs_stage_bytes(int obs_dim, int act_dim, int batch, int64_t M);
/* Form of the last row-split launch on the current device: 0 = gathered in the kernel, 1 = staged inputs, 2 = staged inputs with
 * the x^T operand of layer 1's weight gradient kept as an LDS image (SPO_RS_STAGE=2, A/B form). */
int spo_debug_rs_last_staged(void);
/* The staging pre-pass alone, into out_dev (device memory, 16-byte aligned, out_bytes >= spo_rs_stage_bytes(...)). */
int spo_debug_rs_stage(const float* obs, const float* act, const float* logp_old, const float* target_r, const float* target_c,
                       const float* adv, const int32_t* perm, int64_t M, int obs_dim, int act_dim, int batch, void* out_dev,
                       int64_t out_bytes, void* stream);

/* Seed-batched PPO-Lagrangian: S INDEPENDENT runs (own parameters, optimiser state, buffers, shuffle, cfg scalars) take the
 * minibatch steps of one learning iteration in ONE persistent launch of the row-split kernel, every run on its own six workgroups
 * (3 networks x 2 row groups) of one XCD; run r sits on XCD r mod 8, so up to eight runs have an XCD each and runs r, r + 8, ...
 * share one.  Per run the arithmetic is that of spo_ppo_lag_update_iter on the row-split form, bit for bit.  Every run has its own
 * exchange slots, norm granules, placement census and error word (the int at byte 64 of ITS sync_ws: a run whose exchange timed
 * out leaves its theta and optimiser state as they were and sets it; the others are unaffected).  A run with active == 0 is
 * skipped: nothing of it is read or written.  The launch keeps one ~49 MB scratch block per (device, stream), allocated at the
 * first call together with a pinned host ring of argument tables (not under stream capture; the call itself is not capturable:
 * it copies its argument table from host memory), both freed by spo_update_scratch_release. */
#define SPO_RS_MAX_REPLICAS 32
typedef struct {
  float *theta, *adam_m, *adam_v;
  int64_t adam_step;            /* optimiser steps this run has taken (adam_step_host of spo_ppo_lag_update_iter) */
  const float *obs, *act, *logp_old, *target_r, *target_c, *adv;
  const int32_t* perm;          /* (perm and losses_out may be NULL in a run with active == 0) */
  float* losses_out;            /* [num_minibatches][3] */
  void* sync_ws;                /* >= 72 bytes; only the error word at byte 64 is used */
  spo_ppo_cfg cfg;              /* obs_dim, act_dim, batch equal over the runs; the scalars are the run's own */
  int active;
} spo_update_replica;

/* One learning iteration (ceil(M / batch) steps) for every active run of reps_host[n_replicas] (a HOST array).  Checked on the
 * host before anything is enqueued: 1 <= n_replicas <= SPO_RS_MAX_REPLICAS, equal obs_dim / act_dim / batch, a supported shape
 * (spo_update_rs_multi_supported), no two runs sharing theta or sync_ws.  Does not read SPO_UPDATE_FORM / SPO_RS_OBS128: the
 * caller decides whether to batch.  SPO_RS_SAFE=1 forces write-through exchange stores as in the single launch. */
int spo_ppo_lag_update_iter_multi(const spo_update_replica* reps_host, int n_replicas, int64_t M, void* stream);

/* 1 exactly where (spo_update_rs_supported(D, A, batch, 3) || spo_update_rs128_supported(D, A, batch, 3)) and
 * 1 <= n_replicas <= SPO_RS_MAX_REPLICAS. */
int spo_update_rs_multi_supported(int obs_dim, int act_dim, int batch, int n_replicas);

/* 1 where spo_ppo_lag_update_iter would itself run this shape on the kernel form the seed-batched launch runs (the row-split
 * kernel with two row groups) under this process's routing: SPO_UPDATE_FORM >= 3 and no SPO_RS_ROWS=16 (both read once per
 * process), SPO_RS_OBS128 not 0 above 64 observations.  Batching is bit-for-bit neutral exactly there, so a caller that must
 * reproduce the stand-alone run batches only where this says 1. */
int spo_update_rs_multi_matches_single(int obs_dim, int act_dim, int batch);

/* The launch's block -> (run, workgroup 0..5) mapping, the function the kernel itself uses (testable without a GPU): the grid has
 * 48 * ceil(n_replicas / 8) blocks; block b has XCD label b & 7 and serves run 8 * ((b >> 3) / 6) + (b & 7) as workgroup
 * (b >> 3) % 6.  Returns 1 and fills replica / wg, or 0 for a block without work (run >= n_replicas, or block outside the grid). */
int spo_rs_multi_block_map(int block, int n_replicas, int* replica, int* wg);

/* Measurement aid: {runs that took part in a seed-batched launch, of those: runs whose placement census chose write-through
 * stores (its workgroups not on one XCD, or SPO_RS_SAFE=1)} since the last reset (out2_host, host array).  Their minibatch steps
 * and clipped / redone steps are summed over the runs into spo_debug_update_counters.  Synchronises the device. */
int spo_debug_rs_multi_counters(unsigned long long* out2_host, int reset);

/* Seed-batched critic fit: S INDEPENDENT runs of the CPO family (own critics, optimiser state, buffers, shuffle, cfg scalars,
 * stale actor-gradient norm) take the minibatch steps of one critic-fit iteration in ONE persistent launch of the row-split kernel,
 * every run on its own eight workgroups (2 critics x 4 row groups) of one XCD; run r sits on XCD r mod 8, runs r, r + 8, r + 16
 * share one.  Per run the arithmetic is that of spo_critic_fit_iter on the four-row-group row-split form, bit for bit.  At most
 * 24 runs: three per XCD are 24 working blocks of one CU each on an XCD's 32 CUs -- the 8-CU slack per XCD that co-residency of
 * the PPO form rests on (32 runs would need every CU of every XCD).  Every run has its own exchange slots, norm granules,
 * placement census and error word (the int at byte 64 of ITS sync_ws) and its own stale_sq_io.  A run with active == 0 is skipped:
 * nothing of it is read or written.  The launch keeps one scratch block of its own per (device, stream), sized for 24 runs
 * (24 x 6 MiB of exchange slots + 30 KB of granules and argument table: ~151 MB; the PPO form's block is separate and unchanged),
 * allocated at the first call together with a pinned ring of argument tables (not under stream capture; the call itself is not
 * capturable), freed by spo_update_scratch_release. */
#define SPO_RS_CRITIC_MAX_REPLICAS 24
typedef struct {
  float *theta, *adam_m, *adam_v;
  int64_t adam_step;            /* optimiser steps this run has taken (adam_step_host of spo_critic_fit_iter) */
  const float *obs, *target_r, *target_c;
  const int32_t* perm;          /* (perm and losses_out may be NULL in a run with active == 0) */
  float* losses_out;            /* [num_minibatches][3]; columns 0 and 1 are written */
  float* stale_sq_io;           /* the run's ||actor.grad||^2, in / out (spo_critic_fit_iter); not NULL */
  void* sync_ws;                /* >= 72 bytes: its first 64 bytes are zeroed as spo_critic_fit_iter does, the error word is at byte 64 */
  spo_ppo_cfg cfg;              /* obs_dim, act_dim, batch equal over the runs; the scalars are the run's own */
  int active;
} spo_critic_fit_replica;

/* One critic-fit iteration (ceil(M / batch) steps) for every active run of reps_host[n_replicas] (a HOST array).  Checked on the
 * host before anything is enqueued: 1 <= n_replicas <= SPO_RS_CRITIC_MAX_REPLICAS, equal obs_dim / act_dim / batch, a supported
 * shape (spo_critic_fit_multi_supported), null pointers, no two runs sharing theta, sync_ws or stale_sq_io, a stream under
 * capture.  All runs inactive: returns 0 with nothing enqueued.  Does not read SPO_UPDATE_FORM: the caller decides whether to
 * batch (spo_critic_fit_multi_matches_single).  SPO_RS_SAFE=1 forces write-through exchange stores as in the single launch. */
int spo_critic_fit_iter_multi(const spo_critic_fit_replica* reps_host, int n_replicas, int64_t M, void* stream);

/* 1 exactly where spo_update_rs_supported(D, A, batch, 2), 65 <= batch <= 128 (the four-row-group form; batches up to 64 run
 * two row groups in the single launch and are not batched here) and 1 <= n_replicas <= SPO_RS_CRITIC_MAX_REPLICAS. */
int spo_critic_fit_multi_supported(int obs_dim, int act_dim, int batch, int n_replicas);

/* 1 where spo_critic_fit_iter would itself run this shape on the four-row-group row-split form under this process's routing
 * (SPO_UPDATE_FORM >= 3, read once per process): batching is bit-for-bit neutral exactly there. */
int spo_critic_fit_multi_matches_single(int obs_dim, int act_dim, int batch);

/* The critic-batched launch's block -> (run, workgroup 0..7) mapping, the function the kernel itself uses: the grid has
 * 64 * ceil(n_replicas / 8) blocks; block b has XCD label b & 7 and serves run 8 * ((b >> 3) / 8) + (b & 7) as workgroup
 * (b >> 3) % 8.  Returns 1 and fills replica / wg, or 0 for a block without work (run >= n_replicas, block outside the grid, or
 * n_replicas outside [1, SPO_RS_CRITIC_MAX_REPLICAS]). */
int spo_rs_critic_multi_block_map(int block, int n_replicas, int* replica, int* wg);

/* spo_debug_rs_multi_counters for the critic-batched launches: {runs that took part, of those: on the write-through path} since
 * the last reset.  spo_debug_rs_multi_counters itself counts the PPO launches only, as before.  Synchronises the device. */
int spo_debug_rs_critic_multi_counters(unsigned long long* out2_host, int reset);

/* The row-split kernel's one-GPU forms up to 64 observations skip the joint clip's coefficient arithmetic on a step whose joint squared gradient norm is
 * at most a per-launch threshold, computed on the host from max_grad_norm so that min(1, max_grad_norm / (sqrtf(t) + 1e-6f)) is
 * exactly 1.0f in float32 for every 0 <= t <= threshold (the largest float not above (0.999 max_grad_norm)^2; derivation in
 * csrc/update_rs.hip); above it the exact expression runs as before, so results do not depend on the threshold.  This writes the
 * threshold a launch with this max_grad_norm uses to *thr_sq_out_host: -1 (never taken) below 2e-3, where 0.001 max_grad_norm
 * no longer dominates the 1e-6 and the roundings.  Host code, no GPU.  Refused: a null pointer, a negative or NaN norm.
 * Layer 1's hand-off of the two-row-group forms at 33 .. 64 observations goes out in two batches; SPO_RS_L1_PIPE=0 (read at
 * every launch, by the seed-batched launch too) selects the one-batch form: the same bits, for A/B runs and tests. */
int spo_debug_clip_threshold(float max_grad_norm, float* thr_sq_out_host);

/* Measurement aid: counters of the main + helper update kernel summed over the launches of this process since the last reset
 * (out4_host, host array): {minibatch steps run, steps whose speculative update turned out clipped and was redone, steps
 * clipped under the conservative protocol, steps run under the conservative protocol}.  The row-split kernel adds its steps to
 * the first two; its KIN = 128 form (spo_update_rs128_supported) does not speculate, so nothing is redone there and it adds its
 * steps whose joint clip was active to the second -- the steps a speculating form would have redone.  Synchronises the device. */
int spo_debug_update_counters(unsigned long long* out4_host, int reset);

/* Debug self-test of the cross-lane helpers (DPP row sums, gfx950 permlane swaps): in[64] -> out[192]. */
int spo_debug_crosslane_selftest(const float* in64, float* out192, void* stream);

/* Debug aid (not a reference function): pass a device buffer of 30 u64 to make the next
 * spo_ppo_lag_update_iter launches accumulate shader cycles per phase of the step; NULL disables. */
int spo_debug_set_update_profile(void* dev_u64_30);

/* Split form of the same step for data-parallel training: gradient of ONE
 * minibatch into flat_grad[P] (+ losses[3]); the caller all-reduces flat_grad and then
 * applies clip + Adam.  `grad_scale` multiplies the gradient (1/world_size for averaging). */
int spo_ppo_lag_grad(const float* theta, const float* obs, const float* act, const float* logp_old,
                     const float* target_r, const float* target_c, const float* adv,
                     const int32_t* idx, int n_idx, int64_t mean_count, const spo_ppo_cfg* cfg_host,
                     float* flat_grad, float* losses3, void* stream);
int spo_clip_adam(float* theta, float* adam_m, float* adam_v, const float* flat_grad, int64_t adam_step_host,
                  float grad_scale, const spo_ppo_cfg* cfg_host, void* stream);

/* one host call per data-parallel step: spo_clip_adam(step k) followed by spo_ppo_lag_grad(step k+1)
 * into the same flat_grad buffer (next_idx == NULL: only the optimiser step). */
int spo_clip_adam_then_grad(float* theta, float* adam_m, float* adam_v, float* flat_grad, int64_t adam_step_host,
                            float grad_scale, const float* obs, const float* act, const float* logp_old,
                            const float* target_r, const float* target_c, const float* adv,
                            const int32_t* next_idx, int next_n_idx, const spo_ppo_cfg* cfg_host,
                            float* next_losses3, void* stream);

/* ---- a-11: full-batch actor forward + KL early-stop statistic (ppo_lag.py:277,338-345).
 * spo_actor_mean: mean_out[M,act_dim] = actor.mean(obs).  spo_actor_kl: partial sums of
 * KL(N(mu_old, exp(log_std_old)) || N(mu_new, exp(log_std_new))).sum(-1) over rows into
 * kl_sum (1 double, fixed-order reduction); caller divides by the (global) row count. */
int spo_actor_mean(const float* theta, const float* obs, float* mean_out, int64_t rows,
                   int obs_dim, int act_dim, void* stream);
int spo_actor_kl(const float* theta, const float* obs, const float* mean_old, const float* log_std_old,
                 double* kl_partials, int kl_partials_capacity, double* kl_sum, int64_t rows,
                 int obs_dim, int act_dim, void* stream);

/* ---- CPO (safepo/single_agent/cpo.py).  Actor-only flat vectors use the actor's own layout
 * [log_std, W1, b1, W2, b2, W3, b3] = actor.named_parameters() order (cpo.py:70-78), length
 * Pa = spo_param_count - 2*critic.  Workspaces: partial_ws float[spo_cpo_num_partials(rows)*Pa],
 * loss_ws double[spo_cpo_num_partials(rows)].
 * a-16 spo_cpo_surrogate_grad: grad_out = d/dtheta [ sign * mean(ratio * adv) ], ratio = exp(logp - logp_old)
 *      (cpo.py:356-365 with sign=-1/adv_r, :372-381 with sign=+1/adv_c); loss_sum_out[0] = sum(ratio*adv).
 * a-14 spo_cpo_fvp: out = J^T diag(1/sigma^2) J vec / (rows*act_dim) on the mean-network entries, 0 on the
 *      log_std entries; the caller adds (2/act_dim)*vec[log_std] and the 0.1*vec damping (cpo.py:132-157).
 * a-17 spo_cpo_linesearch_eval: sums3_out = {sum ratio*adv_r, sum ratio*adv_c, sum_{rows,dims} KL(old||new)}
 *      for the parameters currently in theta (cpo.py:473-491).
 * a-18 spo_critic_fit_iter: one pass of the critic fit (cpo.py:541-571) on the persistent kernel with two
 *      networks; *stale_sq_io carries ||actor.grad||^2 (the stale cost gradient that clip_grad_norm_ over ALL
 *      policy parameters still sees, and rescales in place whenever it clips). */
int spo_cpo_num_partials(int64_t rows);
int spo_cpo_surrogate_grad(const float* theta, const float* obs, const float* act, const float* logp_old,
                           const float* adv, float sign, int64_t rows, int obs_dim, int act_dim,
                           float* partial_ws, double* loss_ws, float* grad_out, double* loss_sum_out, void* stream);
int spo_cpo_fvp(const float* theta, const float* obs, const float* vec, int64_t rows, int obs_dim, int act_dim,
                float* partial_ws, double* loss_ws, float* out, void* stream);
int spo_cpo_linesearch_eval(const float* theta, const float* obs, const float* act, const float* logp_old,
                            const float* adv_r, const float* adv_c, const float* mean_old, const float* log_std_old,
                            int64_t rows, int obs_dim, int act_dim, double* partial_ws, int partial_capacity,
                            double* sums3_out, void* stream);

/* ---- CPO full-batch primitives for obs_dim 65..128 (the Car / Racecar / Doggo / Ant tasks of
 * single_agent/benchmark.py:5-44), hidden [64, 64], act_dim <= 16.  Same argument meaning, layouts and workspaces as
 * their namesakes above; obs_dim / act_dim outside that range fail with -2.
 *   spo_cpo128_supported        1 exactly for 65 <= obs_dim <= 128 and 1 <= act_dim <= 16 (host code, no GPU needed)
 *   spo_cpo128_num_partials     workgroups = partial vectors for `rows` rows (sizes partial_ws / loss_ws)
 *   spo_cpo128_surrogate_grad   cpo.py:356-365, :372-381
 *   spo_cpo128_fvp              cpo.py:132-157 (one launch + the fixed-order reduction, like spo_cpo_fvp)
 *   spo_cpo128_linesearch_eval  cpo.py:473-491 */
int spo_cpo128_supported(int obs_dim, int act_dim);
int spo_cpo128_num_partials(int64_t rows);
int spo_cpo128_surrogate_grad(const float* theta, const float* obs, const float* act, const float* logp_old,
                              const float* adv, float sign, int64_t rows, int obs_dim, int act_dim,
                              float* partial_ws, double* loss_ws, float* grad_out, double* loss_sum_out, void* stream);
int spo_cpo128_fvp(const float* theta, const float* obs, const float* vec, int64_t rows, int obs_dim, int act_dim,
                   float* partial_ws, double* loss_ws, float* out, void* stream);
int spo_cpo128_linesearch_eval(const float* theta, const float* obs, const float* act, const float* logp_old,
                               const float* adv_r, const float* adv_c, const float* mean_old, const float* log_std_old,
                               int64_t rows, int obs_dim, int act_dim, double* partial_ws, int partial_capacity,
                               double* sums3_out, void* stream);

/* ---- CPO full-batch primitives for obs_dim 129..512 and act_dim 1..32 (HumanoidVelocity's 376 / 17 in
 * single_agent/benchmark.py:5-44), hidden [64, 64]: W1 is streamed through LDS in 64-feature slices, the output layer is
 * two 16-row tiles.  Same argument meaning, layouts and workspaces as their spo_cpo128_* namesakes; obs_dim / act_dim
 * outside that range fail with -2, naming the dimension, before any device work.
 *   spo_cpo512_supported        1 exactly for 129 <= obs_dim <= 512 and 1 <= act_dim <= 32 (host code, no GPU needed)
 *   spo_cpo512_num_partials     workgroups = partial vectors for `rows` rows (sizes partial_ws / loss_ws)
 *   spo_cpo512_surrogate_grad   cpo.py:356-365, :372-381
 *   spo_cpo512_fvp              cpo.py:132-157 (one launch + the fixed-order reduction)
 *   spo_cpo512_linesearch_eval  cpo.py:473-491
 *   spo_cpo512_actor_mean       cpo.py:361: mean_out[rows, act_dim] = actor.mean(obs), by the forward pass of
 *                               spo_cpo512_linesearch_eval (same products, same order: KL == 0.0 at unchanged parameters) */
int spo_cpo512_supported(int obs_dim, int act_dim);
int spo_cpo512_num_partials(int64_t rows);
int spo_cpo512_surrogate_grad(const float* theta, const float* obs, const float* act, const float* logp_old,
                              const float* adv, float sign, int64_t rows, int obs_dim, int act_dim,
                              float* partial_ws, double* loss_ws, float* grad_out, double* loss_sum_out, void* stream);
int spo_cpo512_fvp(const float* theta, const float* obs, const float* vec, int64_t rows, int obs_dim, int act_dim,
                   float* partial_ws, double* loss_ws, float* out, void* stream);
int spo_cpo512_linesearch_eval(const float* theta, const float* obs, const float* act, const float* logp_old,
                               const float* adv_r, const float* adv_c, const float* mean_old, const float* log_std_old,
                               int64_t rows, int obs_dim, int act_dim, double* partial_ws, int partial_capacity,
                               double* sums3_out, void* stream);
int spo_cpo512_actor_mean(const float* theta, const float* obs, float* mean_out, int64_t rows, int obs_dim, int act_dim,
                          void* stream);

int spo_critic_fit_iter(float* theta, float* adam_m, float* adam_v, int64_t adam_step_host,
                        const float* obs, const float* target_r, const float* target_c, const int32_t* perm,
                        int64_t M, const spo_ppo_cfg* cfg_host, float* stale_sq_io, float* losses_out,
                        void* sync_ws, void* stream);

/* ---- f2: FOCOPS (safepo/single_agent/focops.py:300-350) and CUP (safepo/single_agent/cup.py:300-400) on the
 * persistent update kernel.  spo_update_iter_ex is spo_ppo_lag_update_iter with
 *  - separate Adam step counts for the critics' and the actor's optimisers (CUP's second stage steps the actor alone),
 *  - actor_only != 0: only the actor network is trained and clip_grad_norm_ spans the actor's parameters (cup.py:385),
 *  - actor_loss = SPO_ACTOR_LOSS_CLIP: the PPO clipped surrogate (old_mean/old_std unused, may be NULL), or
 *    SPO_ACTOR_LOSS_KL_PENALTY: loss = mean_i(ind_i*KL_i) - pg_coef*mean_i(ind_i)*mean_j(ratio_j*adv_j) with
 *    KL_i = KL(N(mu_i,sigma) || N(old_mean_i, old_std)).sum(-1), ind_i = [KL_i <= kl_bound]
 *    (focops.py:326-337: kl_bound = target_kl, pg_coef = 1/FOCOPS_LAM; cup.py:372-383: kl_bound = +inf,
 *    pg_coef = -lagrangian_multiplier*(1-gamma*CUP_LAMBDA)/(1-gamma)).  old_mean float[M*act_dim], old_std
 *    float[act_dim].  Needs cfg.batch <= 64.
 * losses_out float[ceil(M/batch)*3]; with actor_only only column 2 is written. */
#define SPO_ACTOR_LOSS_CLIP 0
#define SPO_ACTOR_LOSS_KL_PENALTY 1
int spo_update_iter_ex(float* theta, float* adam_m, float* adam_v, int64_t adam_step_critics_host,
                       int64_t adam_step_actor_host, const float* obs, const float* act, const float* logp_old,
                       const float* target_r, const float* target_c, const float* adv, const int32_t* perm, int64_t M,
                       const spo_ppo_cfg* cfg_host, int actor_loss, const float* old_mean, const float* old_std,
                       float kl_bound, float pg_coef, int actor_only, float* losses_out, void* sync_ws, void* stream);

/* Seed-batched spo_update_iter_ex (FOCOPS, both stages of CUP): S INDEPENDENT runs (own parameters, optimiser state and clocks,
 * buffers, shuffle, old distribution, kl_bound, pg_coef, cfg scalars) take the minibatch steps of one learning iteration in ONE
 * persistent launch of the four-wave kernel, every run on workgroups of its own -- one per network: three, or one with actor_only
 * -- of one XCD; run r sits on XCD r mod 8, runs r, r + 8, ... share one (at most 32 runs: 96 working blocks of one CU each, 12
 * per XCD).  The step is the single launch's, unchanged; per run the result equals spo_update_iter_ex bit for bit wherever that
 * call runs the four-wave kernel itself (spo_update_ex_multi_matches_single).  Every run has its own clip-norm granules (in a
 * block the library owns, ~16 KB per (device, stream) with the argument table, zeroed by one memset per call; allocated at the
 * first call together with a pinned host ring of argument tables, never under stream capture; freed by
 * spo_update_scratch_release) and its own error word, the int at byte 64 of ITS sync_ws; nothing else of sync_ws is touched.  A
 * run with active == 0 is skipped: nothing of it is read or written.  The call copies its argument table from host memory, so it
 * is not capturable and is refused under stream capture. */
#define SPO_UPDATE_EX_MAX_REPLICAS 32
typedef struct {
  float *theta, *adam_m, *adam_v;
  int64_t adam_step_critics, adam_step_actor;   /* the run's two optimiser clocks (spo_update_iter_ex) */
  const float *obs, *act, *logp_old, *target_r, *target_c, *adv;   /* (the targets may be NULL with actor_only) */
  const int32_t* perm;          /* (perm and losses_out may be NULL in a run with active == 0) */
  const float *old_mean, *old_std;              /* (may be NULL with SPO_ACTOR_LOSS_CLIP) */
  float kl_bound, pg_coef;
  float* losses_out;            /* [num_minibatches][3]; with actor_only only column 2 is written */
  void* sync_ws;                /* >= 72 bytes; only the error word at byte 64 is used */
  spo_ppo_cfg cfg;              /* obs_dim, act_dim, batch equal over the runs; the scalars are the run's own */
  int active;
} spo_update_ex_replica;

/* One learning iteration (ceil(M / batch) steps) for every active run of reps_host[n_replicas] (a HOST array); actor_loss and
 * actor_only hold for the whole launch.  Checked on the host before anything is enqueued: 1 <= n_replicas <=
 * SPO_UPDATE_EX_MAX_REPLICAS, equal obs_dim / act_dim / batch, the null pointers spo_update_iter_ex checks, the KL-penalty loss
 * with batch > 64, two runs sharing theta or sync_ws, a stream under capture.  All runs inactive: returns 0 with nothing enqueued.
 * Does not read SPO_UPDATE_FORM: the caller decides whether to batch (spo_update_ex_multi_matches_single). */
int spo_update_iter_ex_multi(const spo_update_ex_replica* reps_host, int n_replicas, int64_t M, int actor_loss, int actor_only,
                             void* stream);

/* 1 for the shapes spo_update_iter_ex accepts (1 <= obs_dim <= SPO_MAX_OBS, 1 <= act_dim <= SPO_MAX_ACT, batch >= 1, and
 * batch <= 64 with the KL-penalty loss) and 1 <= n_replicas <= SPO_UPDATE_EX_MAX_REPLICAS. */
int spo_update_ex_multi_supported(int obs_dim, int act_dim, int batch, int actor_loss, int n_replicas);

/* 1 where spo_update_iter_ex would itself run this shape on the four-wave kernel under this process's routing, so that batching
 * is bit-for-bit neutral: always with the KL-penalty loss; with the clipped surrogate only where the main + helper kernel does
 * not take the launch (obs_dim > 64, or batch > 64, or SPO_UPDATE_FORM < 2; read once per process). */
int spo_update_ex_multi_matches_single(int obs_dim, int act_dim, int batch, int actor_loss);

/* The launch's block -> (run, workgroup) mapping, the function the kernel itself uses (testable without a GPU): with wgs = 1
 * (actor_only) or 3 workgroups per run the grid has 8 * wgs * ceil(n_replicas / 8) blocks; block b has XCD label b & 7 and serves
 * run 8 * ((b >> 3) / wgs) + (b & 7) as workgroup (b >> 3) % wgs.  Returns 1 and fills replica / wg, or 0 for a block without
 * work (run >= n_replicas, block outside the grid, or n_replicas outside [1, SPO_UPDATE_EX_MAX_REPLICAS]). */
int spo_update_ex_multi_block_map(int block, int n_replicas, int actor_only, int* replica, int* wg);

/* Measurement aid: {seed-batched launches enqueued, runs that took part in them} since the last reset (out2_host, host array).
 * Counted on the host when a launch is enqueued: no device access. */
int spo_debug_update_ex_multi_counters(unsigned long long* out2_host, int reset);

/* ---- Data-parallel FOCOPS / CUP: the split form of spo_update_iter_ex (kernel / all-reduce / optimiser per minibatch step).
 * The KL-penalty loss couples every row of a minibatch through F = mean_i(ind_i) (focops.py:326-337: a [B] tensor minus a [B,1]
 * tensor, the mean of a BxB matrix).  Its gradient is linear in F: g_actor = g_KL + F * g_PG with
 *   g_KL = (1/n) sum_i ind_i grad(KL_i),   g_PG = -(pg_coef/n) sum_j grad(ratio_j * adv_j),
 * both row sums, so every rank emits its local parts and one sum all-reduce gives every rank the global F.
 * spo_kl_penalty_grad -- gradient of one local minibatch of n_idx rows (perm indices idx[n_idx], n_idx <= cfg.batch), the
 *   arguments of spo_update_iter_ex otherwise (replaces focops.py:326-347 / cup.py:370-386 up to clip_grad_norm_):
 *   flat_grad float[spo_param_count]: the critics' gradients (mean over the local rows, L2 term and value coefficient included,
 *     as spo_ppo_lag_grad; not written with actor_only) and g_KL in the actor's block (log_std included);
 *   pg_grad float[actor_size]: g_PG taken with F = 1, actor block only (index 0 = log_std[0], the actor's first parameter);
 *   sums float[SPO_KLPEN_SUMS]: {loss_r, loss_c (local minibatch, with L2), count of ind, sum ind*KL, sum ratio*adv, rows}
 *     (with actor_only [0] and [1] are not written).
 *   Every part is a sum over rows, so the sum over the ranks of [flat_grad | pg_grad | sums] (one contiguous buffer) carries the
 *   global minibatch.  Any cfg.batch (no 64-row limit: nothing couples the rows inside a pass).
 * spo_clip_adam_ex -- the optimiser step on the all-reduced buffer, one workgroup (replaces the clip_grad_norm_ + Adam steps of
 *   focops.py:338-347, cup.py:385-386 and of CUP's first stage, cup.py:300-351): grad_scale multiplies every gradient (1/world);
 *   pg_grad != NULL: the actor's gradient is flat_grad + F * pg_grad, F = sums[2] / sums[5]; actor_only: clip norm and Adam over
 *   the actor's parameters only (cup.py:385); separate Adam clocks for the critics and the actor (spo_update_iter_ex).  Adds no
 *   L2 term (the gradient kernels did).  losses3 (optional, needs sums) receives the global minibatch's losses:
 *   {sums[0] * grad_scale, sums[1] * grad_scale (not with actor_only), (sums[3] - pg_coef * F * sums[4]) / sums[5] (pg_grad only)}.
 *   pg_grad == NULL, equal clocks, actor_only == 0: bit-identical to spo_clip_adam.
 * spo_clip_adam_ex_then_kl_grad -- one host call per step: spo_clip_adam_ex (step k) then spo_kl_penalty_grad (step k+1) into the
 *   same buffers (next_idx == NULL: only the optimiser step).
 * spo_clip_adam_ex_then_grad -- the same for the clipped surrogate (CUP's first stage, cup.py:300-351): spo_clip_adam_ex without
 *   the combine (step k), then spo_ppo_lag_grad (step k+1) into flat_grad / next_losses3. */
#define SPO_KLPEN_SUMS 8
int spo_kl_penalty_grad(const float* theta, const float* obs, const float* act, const float* logp_old, const float* target_r,
                        const float* target_c, const float* adv, const int32_t* idx, int n_idx, const spo_ppo_cfg* cfg_host,
                        const float* old_mean, const float* old_std, float kl_bound, float pg_coef, int actor_only,
                        float* flat_grad, float* pg_grad, float* sums, void* stream);
int spo_clip_adam_ex(float* theta, float* adam_m, float* adam_v, const float* flat_grad, const float* pg_grad, const float* sums,
                     int64_t adam_step_critics_host, int64_t adam_step_actor_host, float grad_scale, float pg_coef,
                     int actor_only, const spo_ppo_cfg* cfg_host, float* losses3, void* stream);
int spo_clip_adam_ex_then_grad(float* theta, float* adam_m, float* adam_v, float* flat_grad, int64_t adam_step_critics_host,
                               int64_t adam_step_actor_host, float grad_scale, int actor_only, const float* obs, const float* act,
                               const float* logp_old, const float* target_r, const float* target_c, const float* adv,
                               const int32_t* next_idx, int next_n_idx, const spo_ppo_cfg* cfg_host, float* next_losses3,
                               void* stream);
int spo_clip_adam_ex_then_kl_grad(float* theta, float* adam_m, float* adam_v, float* flat_grad, float* pg_grad, float* sums,
                                  int64_t adam_step_critics_host, int64_t adam_step_actor_host, float grad_scale,
                                  const float* obs, const float* act, const float* logp_old, const float* target_r,
                                  const float* target_c, const float* adv, const float* old_mean, const float* old_std,
                                  float kl_bound, float pg_coef, int actor_only, const int32_t* next_idx, int next_n_idx,
                                  const spo_ppo_cfg* cfg_host, float* losses3, void* stream);

/* ---- (e) multi-GPU, in-kernel form (SURVEY.md 8(e) "direct all-reduce over the xGMI mesh, fused as the epilogue of
 * the backward kernel").  Each rank owns one exchange region (uncached device memory, spo_p2p_alloc) and maps its
 * peers' regions through the 64-byte IPC handle (spo_p2p_open; exchange the handles with any host collective).
 * regions[r] = rank r's region as seen from this process (own pointer at index rank), world <= 8.
 * spo_ppo_lag_update_iter_dp is spo_ppo_lag_update_iter for one rank of a data-parallel job: every rank launches it on
 * its own shard (same M, same batch, same step counts) and the per-step mean of the ranks' minibatch gradients is formed
 * inside the step, so all replicas apply bit-identical updates.  Every float travels as an 8-byte {tag, value} word
 * written with one system-scope write-through store and polled by the lane that needs it (no flags, no barriers):
 * power-of-two worlds use recursive doubling (round k: swap the running sum with rank me ^ 2^k; log2(world) hand-offs);
 * other worlds reduce-scatter then all-gather (two hand-offs, 2 x 88 KB per network per step).  Environment:
 * SPO_P2P_ALGO=twophase forces the second form everywhere.  step0 = optimiser steps already taken through these regions (monotonic tag base, identical
 * on every rank; advance it by the number of minibatches).  A peer that never answers costs ONE bounded wait and is
 * reported through sync_ws (int at byte 64 = 2), never a hang.
 * spo_p2p_selftest runs `iters` exchange rounds of known patterns on the same grid and protocol:
 * result2_dev[0] = wrong values, result2_dev[1] = 2 after a timeout; it consumes `iters` tags. */
int64_t spo_p2p_region_bytes(void);
int spo_debug_xr_profile(unsigned long long* out8_host, int reset);

/* spo_ppo_lag_update_iter for wide observations / action vectors (round 5; csrc/update_ks.hip): obs_dim <= 512, act_dim <= 32,
 * batch <= 64, hidden [64, 64], the clipped-surrogate loss, one GPU.  The first layer is split over the input features, 64 per
 * workgroup: 3 x ceil(obs_dim / 64) persistent workgroups exchange the partial pre-activations inside the step; same
 * arguments, results and per-step loss log as spo_ppo_lag_update_iter (reference: safepo/single_agent/ppo_lag.py:297-336 with
 * an ActorVCritic(376, 17), model.py:131; single_agent/benchmark.py:5-22).  spo_ks_supported: 1 when the shape fits. */
int spo_ks_supported(int obs_dim, int act_dim, int batch);
int spo_ppo_lag_update_iter_ks(float* theta, float* adam_m, float* adam_v, int64_t adam_step_host, const float* obs,
                               const float* act, const float* logp_old, const float* target_r, const float* target_c,
                               const float* adv, const int32_t* perm, int64_t M, const spo_ppo_cfg* cfg_host,
                               float* losses_out, void* sync_ws, void* stream);
/* spo_update_iter_ex on the feature-split kernel: the KL-penalty actor loss of FOCOPS (focops.py:326-337) and CUP's second stage
 * (cup.py:372-383), separate optimiser clocks, actor-only mode -- same arguments and semantics as spo_update_iter_ex, shapes as
 * spo_ks_supported, one GPU. */
int spo_update_iter_ex_ks(float* theta, float* adam_m, float* adam_v, int64_t adam_step_critics_host,
                          int64_t adam_step_actor_host, const float* obs, const float* act, const float* logp_old,
                          const float* target_r, const float* target_c, const float* adv, const int32_t* perm, int64_t M,
                          const spo_ppo_cfg* cfg_host, int actor_loss, const float* old_mean, const float* old_std,
                          float kl_bound, float pg_coef, int actor_only, float* losses_out, void* sync_ws, void* stream);

/* Seed-batched spo_update_iter_ex_ks (the six first-order scripts at HumanoidVelocity-class dims): S INDEPENDENT runs (own
 * parameters, optimiser state and clocks, buffers, shuffle, old distribution, kl_bound, pg_coef, cfg scalars) take the minibatch
 * steps of one learning iteration in ONE launch of the feature-split kernel, every run on workgroups of its own -- (3, or 1 with
 * actor_only) x ceil(obs_dim / 64) -- of one XCD; run r sits on XCD label r mod 8, runs r and r + 8 share one.  Per run the
 * semantics and the bits are spo_update_iter_ex_ks's (actor_loss == SPO_ACTOR_LOSS_CLIP with equal clocks:
 * spo_ppo_lag_update_iter_ks's).  Every run has its own exchange slots, granules and placement census in a block the library owns
 * (16 x 7 090 176 bytes + the argument table = 113 449 344 bytes per (device, stream), separate from the single launch's scratch;
 * allocated at the first call together with a pinned host ring of argument tables, never under stream capture; freed by
 * spo_update_scratch_release) and its own error word, the int at byte 64 of ITS sync_ws; nothing else of sync_ws is touched.  A
 * run whose exchange times out leaves its parameters and optimiser state untouched and sets its error word; the other runs are
 * unaffected.  A run with active == 0 is skipped: nothing of it is read or written.  Checked on the host before anything is
 * enqueued: the replica range (spo_update_ks_multi_supported), equal obs_dim / act_dim / batch, the null pointers
 * spo_update_iter_ex_ks checks, non-negative clocks, two runs sharing theta or sync_ws, a stream under capture (the argument
 * table is copied from host memory at every call), ceil(M / batch) < 2^30.  All runs inactive: returns 0 with nothing enqueued.
 * SPO_KS_SAFE is read as in the single launch; SPO_WIDE_KS is not: the caller decides whether to batch. */
#define SPO_KS_MAX_REPLICAS 16
int spo_update_iter_ex_ks_multi(const spo_update_ex_replica* reps_host, int n_replicas, int64_t M, int actor_loss, int actor_only,
                                void* stream);

/* 1 where spo_ks_supported(obs_dim, act_dim, batch) and 1 <= n_replicas <= min(SPO_KS_MAX_REPLICAS, 8 * (8 / S)) with
 * S = ceil(obs_dim / 64) and integer division: at most 24 working blocks per XCD label, each on one of that XCD's 32 CUs, so all
 * workgroups of the launch are co-resident -- 16 runs up to 256 observations, 8 at 257 .. 512.  A run counts as 3 S blocks
 * whatever actor_only is (one cap for both stages of CUP). */
int spo_update_ks_multi_supported(int obs_dim, int act_dim, int batch, int n_replicas);

/* The launch's block -> (run, workgroup) mapping, the function the kernel itself uses (testable without a GPU): with
 * wgs = (actor_only ? 1 : 3) * ceil(obs_dim / 64) workgroups per run the grid has 8 * wgs * ceil(n_replicas / 8) blocks; block b
 * has XCD label b & 7 and serves run 8 * ((b >> 3) / wgs) + (b & 7) as workgroup (b >> 3) % wgs.  Returns 1 and fills replica /
 * wg, or 0 for a block without work (run >= n_replicas, block outside the grid, or n_replicas outside the supported range). */
int spo_update_ks_multi_block_map(int block, int obs_dim, int n_replicas, int actor_only, int* replica, int* wg);

/* Measurement aid: {seed-batched launches enqueued, runs that took part in them, of those: runs whose placement census chose
 * write-through exchange stores} since the last reset (out3_host, host array).  The third is counted by the kernel in a word per
 * run; the call synchronises the device to read it. */
int spo_debug_update_ks_multi_counters(unsigned long long* out3_host, int reset);

/* One minibatch's gradient on the feature-split kernel (round 6: the data-parallel step at these dims): the RAW
 * data gradient (no L2 term, no value coefficient) of the three networks on rows idx[0 .. n), n <= 64, into flat_grad (theta's
 * layout, log_std included) and the three data losses into losses3 -- ppo_lag.py:306-324 up to loss.backward(), the part
 * spo_mlp_forward / spo_wide_ppo_loss / spo_mlp_backward take 20 launches for.  theta is not written.  The caller averages
 * flat_grad over the ranks (the global minibatch is the concatenation of the ranks' rows; the reference itself is one process) and
 * applies spo_wide_clip_adam. */
int spo_ppo_lag_grad_ks(const float* theta, const float* obs, const float* act, const float* logp_old, const float* target_r,
                        const float* target_c, const float* adv, const int32_t* idx, int n, const spo_ppo_cfg* cfg_host,
                        float* flat_grad, float* losses3, void* sync_ws, void* stream);
/* spo_critic_fit_iter on the same feature-split kernel (two networks): the critic fit of the second-order scripts
 * (safepo/single_agent/cpo.py:541-571) for obs_dim <= 512, hidden [64, 64], batch <= 128 (a minibatch is taken as two 64-column
 * chunks whose gradients accumulate before the optimiser step), one GPU.  Same arguments and results as spo_critic_fit_iter;
 * cfg_host->act_dim only locates the critics in the flat parameter vector. */
int spo_critic_fit_ks_supported(int obs_dim, int batch);
int spo_critic_fit_iter_ks(float* theta, float* adam_m, float* adam_v, int64_t adam_step_host, const float* obs,
                           const float* target_r, const float* target_c, const int32_t* perm, int64_t M,
                           const spo_ppo_cfg* cfg_host, float* stale_sq_io, float* losses_out, void* sync_ws, void* stream);

/* Seed-batched spo_critic_fit_iter_ks (the six second-order scripts at HumanoidVelocity-class dims): one critic-fit iteration
 * (ceil(M / batch) steps) for every active run of reps_host[n_replicas] (a HOST array of the spo_critic_fit_replica records
 * spo_critic_fit_iter_multi takes) in ONE launch of the feature-split kernel, every run on its own 2 x ceil(obs_dim / 64)
 * workgroups of one XCD; run r sits on XCD label r mod 8, runs r and r + 8 share one.  Per run the arithmetic is
 * spo_critic_fit_iter_ks's, bit for bit (the two 64-column chunks of a 65-128-row minibatch, the stale actor-gradient norm in the
 * joint clip, the placement census, SPO_KS_SAFE).  Every run has its own exchange slots, granules and census words -- in the block
 * spo_update_iter_ex_ks_multi keeps per (device, stream), which both launches share: launches on one stream are ordered and each
 * primes the slots of its active runs -- its own stale_sq_io and its own error word, the int at byte 64 of ITS sync_ws.  Unlike
 * spo_critic_fit_iter_ks, which zeroes the first 64 bytes of sync_ws, this launch touches nothing else of sync_ws (the kernel reads
 * none of it).  A run whose exchange times out leaves its parameters and optimiser state untouched and sets its error word; the
 * other runs are unaffected.  A run with active == 0 is skipped: nothing of it is read or written (its perm / losses_out may be
 * NULL).  Refused on the host before anything is enqueued, each with its own message: a null table, n_replicas outside
 * [1, SPO_KS_MAX_REPLICAS] or the shape's cap (spo_critic_fit_ks_multi_supported), M <= 0, unequal obs_dim / act_dim / batch, a shape
 * outside spo_critic_fit_ks_supported, act_dim < 1, null pointers of an active run, stale_sq_io NULL, a negative adam_step, two
 * runs sharing theta, sync_ws or stale_sq_io, ceil(M / batch) >= 2^30, a stream under capture.  All runs inactive: returns 0 with
 * nothing enqueued.  SPO_WIDE_KS is not read: the caller decides whether to batch. */
int spo_critic_fit_iter_ks_multi(const spo_critic_fit_replica* reps_host, int n_replicas, int64_t M, void* stream);

/* 1 where spo_critic_fit_ks_supported(obs_dim, batch) and 1 <= n_replicas <= min(SPO_KS_MAX_REPLICAS, 8 * (24 / (2 * S))) with
 * S = ceil(obs_dim / 64) and integer division: at most 24 working blocks per XCD label, each on one of that XCD's 32 CUs, a run
 * being 2 S blocks -- 16 runs up to 384 observations (HumanoidVelocity's 376 included), 8 at 385 .. 512. */
int spo_critic_fit_ks_multi_supported(int obs_dim, int batch, int n_replicas);

/* The launch's block -> (run, workgroup) mapping, the function the kernel itself uses (testable without a GPU): with
 * wgs = 2 * ceil(obs_dim / 64) the grid has 8 * wgs * ceil(n_replicas / 8) blocks; block b has XCD label b & 7 and serves run
 * 8 * ((b >> 3) / wgs) + (b & 7) as workgroup (b >> 3) % wgs.  Returns 1 and fills replica / wg (both optional), or 0 for a block
 * without work (run >= n_replicas, block outside the grid, or n_replicas outside the supported range). */
int spo_critic_fit_ks_multi_block_map(int block, int obs_dim, int n_replicas, int* replica, int* wg);

/* Measurement aid: {spo_critic_fit_iter_ks_multi launches enqueued, runs that took part in them, of those: runs whose placement
 * census chose write-through exchange stores} since the last reset (out3_host, host array).  The third is counted by the kernel
 * in a word per run of its own, beside the one spo_debug_update_ks_multi_counters reads (which keeps counting the first-order
 * launches only); the call synchronises the device to read it. */
int spo_debug_critic_fit_ks_multi_counters(unsigned long long* out3_host, int reset);

/* Form of the in-kernel gradient exchange (which of the built all-reduce forms runs inside the persistent update
 * kernel).  spo_p2p_select_form pins one for the process (-1: back to the default policy: environment overrides, else the row-split
 * form at 2 / 4 / 8 ranks -- shapes outside the row-split kernel run the four-wave kernel -- recursive doubling at 2 / 4 ranks and
 * the two-phase form elsewhere); a form that does not exist at a world size falls back to the policy.
 * safepo.parallel.PeerExchange.autotune times every valid form at start-up on the actual topology and pins the fastest. */
#define SPO_XR_FORM_TWOPHASE 0          /* packed reduce-scatter + all-gather, four-wave kernel: two hand-offs at any world size   */
#define SPO_XR_FORM_DOUBLING 1          /* packed recursive doubling, four-wave kernel: log2(world) hand-offs (power-of-two worlds) */
#define SPO_XR_FORM_HELPER_A2A 2        /* one-shot all-to-all with flags on the helper waves (worlds 2 / 4 / 8): one hand-off      */
#define SPO_XR_FORM_HELPER_DOUBLING 3   /* packed recursive doubling on the helper waves, layer by layer (worlds 2 / 4 / 8)          */
#define SPO_XR_FORM_ROW_SPLIT 4         /* round 6: the row-split kernel (spo_update_rs_supported), tagged 16-byte words behind the row
                                         * groups' L2 hand-off.  2 ranks: the gradient goes to the peer at once (ONE cross-rank hand-off);
                                         * 4 / 8 ranks: reduce-scatter + all-gather -- every word to its owner rank, which adds the
                                         * world's contributions in rank order (all polled in one batch) and sends the finished word to
                                         * everyone: two hand-offs on world - 1 links each (SPO_P2P_ALGO=rowsplit)                     */
int spo_p2p_select_form(int form);
int spo_p2p_form_valid(int form, int world);
int spo_p2p_current_form(int world);

/* self-test kernel phase cycles (debug) */
int spo_p2p_alloc(void** region_out, void* ipc_handle64_out);
int spo_p2p_open(const void* ipc_handle64, void** region_out);
int spo_p2p_close(void* peer_region);
int spo_p2p_free(void* own_region);
int spo_p2p_selftest(int rank, int world, void* const* regions, uint32_t step0, int iters, int32_t* result2_dev,
                     void* stream);
int spo_critic_fit_iter_dp(float* theta, float* adam_m, float* adam_v, int64_t adam_step_host, const float* obs,
                           const float* target_r, const float* target_c, const int32_t* perm, int64_t M,
                           const spo_ppo_cfg* cfg_host, float* stale_sq_io, float* losses_out, void* sync_ws, int rank,
                           int world, void* const* regions, uint32_t step0, void* stream);
/* One-grid split critic fit (single GPU; cpo.py:534-571 at batch_size 128): the two 64-row halves of every minibatch run on
 * two workgroup pairs of ONE launch, each with its own replica (theta0/1, adam_m0/1, adam_v0/1, stale_sq_io0/1, losses0/1,
 * sync_ws0/1) and its own rows (perm0 / perm1: M_half entries each), exchanging the gradient inside the step through
 * regions2[0..1] (spo_p2p_alloc; no IPC).  Co-resident by construction -- no second stream.  Consumes ceil(M_half / batch)
 * tags from step0.  spo_p2p_selftest_one_grid: the exchange self-test in the same one-grid shape, result4_dev =
 * {wrong values, timeout} per rank. */
int spo_critic_fit_iter_split(float* theta0, float* adam_m0, float* adam_v0, float* theta1, float* adam_m1, float* adam_v1,
                              int64_t adam_step_host, const float* obs, const float* target_r, const float* target_c,
                              const int32_t* perm0, const int32_t* perm1, int64_t M_half, const spo_ppo_cfg* cfg_host,
                              float* stale_sq_io0, float* stale_sq_io1, float* losses0, float* losses1, void* sync_ws0,
                              void* sync_ws1, void* const* regions2, uint32_t step0, void* stream);
int spo_p2p_selftest_one_grid(void* const* regions2, uint32_t step0, int iters, int32_t* result4_dev, void* stream);

/* Seed-batched one-grid split critic fit (cpo.py:534-571 at batch_size 128 and 65-128 observations -- the Car / Racecar / Doggo /
 * Ant tasks of the default sweep, single_agent/benchmark.py:5-44): the spo_critic_fit_iter_split launches of S INDEPENDENT runs
 * (own critics and second replica, optimiser state, buffers, shuffle, cfg scalars, stale actor-gradient norms, exchange regions,
 * step tag) as ONE persistent launch per critic-fit iteration.  Run r has four workgroups of its own on XCD label r mod 8
 * (workgroups 0, 1: the first replica's two critics on rows perm0; 2, 3: the second's on perm1), runs r, r + 8, ... share an XCD.
 * Per run the arithmetic is spo_critic_fit_iter_split's, bit for bit: the same step body and the same placement census, taken per
 * run -- a run whose four workgroups sit on one XCD exchanges through that XCD's L2 (a cached pair of regions the library owns),
 * any other through its own uncached pair regions2[0..1]; SPO_CPO_SPLIT_L2=0 puts every run on the uncached pair.  At most 32
 * runs: four per XCD are 16 working blocks of one CU each on an XCD's 32 CUs (the other batched launches stop at 24).
 * The library keeps one block per (device, stream) for this launch: per run a cached pair of exchange regions (the prefix the
 * world-2 doubling form touches, 2 x 3 194 880 bytes), the clip-norm granules of both replicas (256 bytes), 256 bytes of census
 * words and a census tag, then the argument table -- 6 390 016 cleared bytes per run, 204.5 MB at 32 runs; allocated at the first
 * call and grown to the largest S seen (never under stream capture; the call itself is refused there: its argument table is
 * copied from host memory), cleared for the S runs of a launch by one memset, freed by spo_update_scratch_release.
 * Of sync_ws0 / sync_ws1 only the error words (the int at byte 64) are used.  A run with active == 0 is skipped: nothing of it is
 * read or written, and its pointers may be NULL. */
#define SPO_CRITIC_SPLIT_MAX_REPLICAS 32
typedef struct {
  float *theta0, *adam_m0, *adam_v0;       /* first replica: the run's own parameters and moments */
  float *theta1, *adam_m1, *adam_v1;       /* second replica: a copy of the first at the start of the critic fit */
  int64_t adam_step;                       /* optimiser steps this run has taken (adam_step_host of spo_critic_fit_iter_split) */
  const float *obs, *target_r, *target_c;
  const int32_t *perm0, *perm1;            /* M_half rows each: columns 0-63 / 64-127 of every 128-row minibatch */
  float *stale_sq_io0, *stale_sq_io1;      /* ||actor.grad||^2 of both replicas, in / out */
  float *losses0, *losses1;                /* [ceil(M_half / batch)][3] each; columns 0 and 1 are written */
  void *sync_ws0, *sync_ws1;               /* >= 72 bytes each; only the error word at byte 64 is used */
  void* regions2[2];                       /* the run's uncached pair (spo_p2p_alloc) */
  uint32_t step0;                          /* the run's step tag; the launch consumes ceil(M_half / batch) tags from it */
  spo_ppo_cfg cfg;                         /* obs_dim, act_dim, batch (rows per half, <= 64) equal over the runs */
  int active;
} spo_critic_fit_split_replica;

/* One critic-fit iteration (ceil(M_half / batch) steps) for every active run of reps_host[n_replicas] (a HOST array).  Checked on
 * the host before anything is enqueued: a null table, 1 <= n_replicas <= SPO_CRITIC_SPLIT_MAX_REPLICAS, M_half > 0, equal obs_dim
 * / act_dim / batch, a supported shape (spo_critic_fit_split_multi_supported), null pointers and a negative adam_step of an active
 * run, two runs sharing theta or sync_ws (either replica), a run whose two replicas alias, a stream under capture.  All runs
 * inactive: returns 0 with nothing enqueued. */
int spo_critic_fit_iter_split_multi(const spo_critic_fit_split_replica* reps_host, int n_replicas, int64_t M_half, void* stream);

/* 1 for 65 <= obs_dim <= 128 (the KIN = 128 form; up to 64 observations default routing never takes the split form and
 * spo_critic_fit_iter_multi covers the range), 1 <= batch <= 64 (rows per half) and 1 <= n_replicas <=
 * SPO_CRITIC_SPLIT_MAX_REPLICAS. */
int spo_critic_fit_split_multi_supported(int obs_dim, int batch, int n_replicas);

/* The launch's block -> (run, workgroup 0..3) mapping, the function the kernel itself uses: the grid has 32 * ceil(n_replicas / 8)
 * blocks; block b has XCD label b & 7 and serves run 8 * ((b >> 3) / 4) + (b & 7) as workgroup (b >> 3) % 4.  Returns 1 and fills
 * replica / wg, or 0 for a block without work (run >= n_replicas, block outside the grid, or n_replicas outside the cap). */
int spo_critic_fit_split_multi_block_map(int block, int n_replicas, int* replica, int* wg);

/* Measurement aid: {launches enqueued, runs that took part, of those: runs whose census chose the shared-L2 body} since the last
 * reset (out3_host, host array).  The first two are counted on the host; the third is a word per run the kernel stores into,
 * read back here (synchronises the device once a launch has been made). */
int spo_debug_critic_fit_split_multi_counters(unsigned long long* out3_host, int reset);
int spo_ppo_lag_update_iter_dp(float* theta, float* adam_m, float* adam_v, int64_t adam_step_host, const float* obs,
                               const float* act, const float* logp_old, const float* target_r, const float* target_c,
                               const float* adv, const int32_t* perm, int64_t M, const spo_ppo_cfg* cfg_host,
                               float* losses_out, void* sync_ws, int rank, int world, void* const* regions,
                               uint32_t step0, void* stream);

/* ---- multi-agent masked GAE: SeparatedReplayBuffer.compute_returns + compute_cost_returns
 * (safepo/common/buffer.py:356-384) with PopArt.denormalize (safepo/common/popart.py:117-133) folded in.
 * Time-major arrays as in the reference: rewards/costs [T, N], value_preds/cost_preds/masks [T+1, N] (row T =
 * bootstrap value / last mask), returns/cost_returns [T+1, N] (rows 0..T-1 written).  fp32, the reference's
 * operation order: results are bit-identical.  denorm_std = sqrt(debiased var), denorm_mean = debiased mean
 * (pass 1, 0 when no value normaliser is used). */
int spo_ma_gae(const float* rewards, const float* costs, const float* value_preds, const float* cost_preds,
               const float* masks, float* returns, float* cost_returns, int64_t T, int64_t num_threads,
               double gamma, double gae_lambda, float denorm_std_r, float denorm_mean_r,
               float denorm_std_c, float denorm_mean_c, void* stream);

/* parameter-vector geometry helpers (host) */
int64_t spo_param_count(int obs_dim, int act_dim);
int64_t spo_param_offset(int obs_dim, int act_dim, int net /*0 r-critic,1 c-critic,2 actor*/);

/* ---- bench/test utility (NOT a reference function): device-resident synthetic env
 * (SURVEY.md 8d): obs'~N(0,1), reward~N(0,1), cost~Bernoulli(p_cost), terminated~Bernoulli(p_term),
 * truncated = episode length >= trunc_len; counter-based RNG keyed by (seed, step, env). */
int spo_synth_env_step(float* next_obs, float* final_obs, float* reward, float* cost, float* terminated,
                       float* truncated, int* t_env, int64_t num_envs, int obs_dim, uint64_t seed,
                       uint64_t step, float p_term, float p_cost, int trunc_len, void* stream);

/* The same with the step counter split into a device-resident base and a host offset: step = *step_base_dev + step_rel.  A launch
 * captured into a HIP graph (step_rel = the index inside the epoch) then draws fresh numbers at every replay once the host has
 * moved *step_base_dev to the epoch's first step (the collect loop as one graph replay, safepo/common/engine.py).  One launch;
 * affine != 0: next_obs = fl(fl(x * obs_scale) + obs_shift), the raw-observation map of SynthDeviceEnv (obs <= 1024 columns). */
int spo_synth_env_step_rel(float* next_obs, float* final_obs, float* reward, float* cost, float* terminated,
                           float* truncated, int* t_env, int64_t num_envs, int obs_dim, uint64_t seed,
                           uint64_t step_rel, const uint64_t* step_base_dev, float p_term, float p_cost, int trunc_len,
                           int affine, float obs_scale, float obs_shift, void* stream);

/* ---- f3: multi-agent MAPPO-L networks and update (csrc/ma_net.hip; plain products: csrc/gemm_f32.hip).
 * Networks: safepo/common/model.py:172-363 + safepo/utils/{mlp,act,distributions}.py -- LayerNorm(obs), then n_blocks x
 * [Linear -> ELU -> LayerNorm], then a Linear head (actor: action mean, with a state-independent
 * std = sigmoid(log_std / std_x_coef) * std_y_coef; critics: one value).  One flat fp32 parameter vector per network in the
 * reference's state_dict order (spo_ma_param_offset: which = 0 feature_norm.weight, 1 feature_norm.bias, 2 W_k, 3 b_k,
 * 4 ln_k.weight, 5 ln_k.bias, 6 log_std, 7 head W, 8 head b).  GEMMs run on the in-tree fp32 MFMA kernels.
 * spo_ma_forward keeps the activations of `rows` rows in ws (spo_ma_workspace_floats) for spo_ma_backward, which turns
 * d(loss)/d(head output) into the flat gradient (log_std's entry is owned by spo_ma_actor_loss).
 * Trainer pieces (safepo/multi_agent/mappolag.py:126-199): spo_ma_actor_loss = clipped surrogate on
 * imp = prod_a exp(logp_a - old_a) with the hybrid advantage adv - lamda*cost_adv, HAPPO factor, active masks and entropy
 * bonus; scalars5_out = {policy_loss, dist_entropy, mean(imp), mean(imp*cost_adv), sum(active)};
 * spo_ma_lamda_update = the in-loop multiplier step; spo_ma_popart_forward = PopArt.forward (popart.py:86-112) on a
 * [rows] vector, state3 = {running_mean, running_mean_sq, debiasing_term}; spo_ma_value_loss = max of the clipped /
 * unclipped Huber losses (util.huber_loss, including its zero branch for e < -delta) with separately normalised targets;
 * spo_ma_clip_adam = clip_grad_norm_ + torch.optim.Adam(lr, eps, weight_decay) on one network.
 * HAPPO / MAPPO (safepo/multi_agent/{happo,mappo}.py) run on the same entry points: no cost critic / multiplier (pass
 * lamda = 0), spo_ma_value_loss with active_or_null != NULL and denom_host = the global sum of active masks for
 * use_value_active_masks (else NULL and the global row count), and per_dim_ratio = 1 for MAPPO's per-dimension ratios.
 * Data parallel over rollout threads: every mean is taken over the GLOBAL batch -- denom_host (global row count, or the
 * global sum of active masks) and rows_global are passed in, scalars / losses come back as this rank's share of the
 * global mean, and the caller all-reduces (sum) the scalars, the PopArt sums and the flat gradients before
 * spo_ma_lamda_update / spo_ma_popart_forward / spo_ma_clip_adam.  Single rank: rows_global = rows. */
typedef struct spo_ma_net {
  int32_t in_dim, hidden, n_blocks, out_dim, is_actor;
} spo_ma_net;
typedef struct spo_ma_loss_cfg {
  float clip_param, entropy_coef, std_x_coef, std_y_coef;
  int32_t use_policy_active_masks;
  int32_t per_dim_ratio;      /* MAPPO (mappo.py:150-160): per-dimension ratios, min(surr1, surr2) summed over dimensions */
} spo_ma_loss_cfg;
int64_t spo_ma_param_count(const spo_ma_net* net);
int64_t spo_ma_param_offset(const spo_ma_net* net, int which, int block);
int64_t spo_ma_workspace_floats(const spo_ma_net* net, int64_t rows);
int64_t spo_ma_backward_scratch_floats(const spo_ma_net* net, int64_t rows);
int spo_ma_forward(const float* theta, const spo_ma_net* net, const float* x, int64_t rows, float* ws, float* out,
                   void* stream);
int spo_ma_backward(const float* theta, const spo_ma_net* net, const float* x, int64_t rows, const float* ws,
                    const float* dout, float* grad, float* scratch, void* stream);
/* Tangent (forward-mode) pass of the same network: dout[rows, out_dim] = d(out)/d(theta) . tangent at the point whose
 * activations spo_ma_forward left in ws (tangent: flat, laid out like theta; a log_std slot is ignored).  With
 * spo_ma_backward this gives MACPO's Fisher-vector product J^T M J v without a second-order autograd pass
 * (replaces the double torch.autograd.grad of safepo/multi_agent/macpo.py:187-199).
 * scratch: float[spo_ma_jvp_scratch_floats(net, rows)]. */
int64_t spo_ma_jvp_scratch_floats(const spo_ma_net* net, int64_t rows);
int spo_ma_jvp(const float* theta, const spo_ma_net* net, const float* tangent, int64_t rows, const float* ws, float* dout,
               float* scratch, void* stream);
/* Insert of one environment step into the per-agent buffers (Runner.insert, mappolag.py:449-492) as ONE launch: the
 * environment's [threads, agents, ...] observations / shared observations / rewards / costs are written to every agent's
 * time-major buffer row, masks and active masks are formed from the done flags (dones: [threads, agents] bytes, non-zero =
 * done): masks = 0 where all agents of the thread are done, active_masks = 0 for a done agent of a thread that is not.
 * Each *_dst addresses the row of agent 0 at the step slot being filled ([threads, dim] contiguous); *_agent_stride is the
 * distance in floats to the same row of the next agent.  costs / costs_dst may both be NULL (happo / mappo). */
int spo_ma_insert_step(const float* obs, const float* share_obs, const float* rewards, const float* costs,
                       const unsigned char* dones, float* obs_dst, int64_t obs_agent_stride, float* share_obs_dst,
                       int64_t share_obs_agent_stride, float* rewards_dst, int64_t rewards_agent_stride, float* costs_dst,
                       int64_t costs_agent_stride, float* masks_dst, int64_t masks_agent_stride, float* active_masks_dst,
                       int64_t active_masks_agent_stride, int64_t num_threads, int32_t num_agents, int32_t obs_dim,
                       int32_t share_obs_dim, void* stream);
/* Collect step of the multi-agent runner (mappolag.py:411-447: policy.get_actions for every agent): ALL networks of ALL
 * agents in one launch, each 64-row tile taken through its whole network on chip (feature LayerNorm, blocks, head, and for
 * actors the Gaussian sample + per-dimension log-probabilities).  Results are bit-identical to spo_ma_forward (+
 * spo_ma_sample) per network.  Geometry served: hidden 128, in_dim <= 128 and a multiple of 4, out_dim <= 16, n_blocks <= 4,
 * n_nets <= SPO_MA_COLLECT_MAX_NETS, 16-byte aligned theta / x; anything else returns SPO_MA_COLLECT_UNSUPPORTED without
 * launching (the caller then runs the per-network entry points).
 * critics: out[rows, 1] required.  actors: act / logp [rows, out_dim] required, eps [rows, out_dim] unless deterministic,
 * out (the mean) optional.  scratch: float[spo_ma_collect_scratch_floats(n_nets)] (folded first-block weights). */
#define SPO_MA_COLLECT_MAX_NETS 16
#define SPO_MA_COLLECT_UNSUPPORTED 1
typedef struct spo_ma_collect_net {
  const float* theta;
  spo_ma_net net;
  int32_t deterministic;
  const float* x;
  float* out;
  const float* eps;
  float* act;
  float* logp;
  float std_x_coef, std_y_coef;
} spo_ma_collect_net;
int64_t spo_ma_collect_scratch_floats(int32_t n_nets);
int spo_ma_collect_forward(int32_t n_nets, const spo_ma_collect_net* nets, int64_t rows, float* scratch, void* stream);
int spo_ma_sample(const float* mean, const float* log_std, const float* eps, float std_x_coef, float std_y_coef,
                  int deterministic, float* act_out, float* logp_out, int64_t rows, int act_dim, void* stream);
int spo_ma_log_probs(const float* mean, const float* log_std, const float* act, float std_x_coef, float std_y_coef,
                     float* logp_out, int64_t rows, int act_dim, void* stream);
int spo_ma_actor_loss(const float* mean, const float* log_std, const float* act, const float* old_logp, const float* adv,
                      const float* cost_adv, const float* factor, const float* active, const float* lamda_dev,
                      const spo_ma_loss_cfg* cfg, int64_t rows, int act_dim, float denom_host, int64_t rows_global,
                      float* dmean_out, float* dlogstd_out, float* scalars5_out, double* partial_ws, void* stream);
int spo_ma_lamda_update(float* lamda_dev, const float* scalars5, float aver_episode_cost, float cost_limit, float gamma,
                        float lagrangian_coef_rate, void* stream);
int spo_ma_popart_stats(const float* x, int64_t rows, double* sums2_dev, double* partial_ws, void* stream);
int spo_ma_popart_forward(const float* x, int64_t rows, float* state3, double beta, float epsilon, int train,
                          const double* sums2_dev, int64_t rows_global, float* out, void* stream);
int spo_ma_value_loss(const float* values, const float* value_preds, const float* returns_norm_clipped,
                      const float* returns_norm_original, const float* active_or_null, float denom_host, float clip_param,
                      float huber_delta, float value_loss_coef, int64_t rows, int64_t rows_global, float* dvalues_out,
                      float* loss_out, double* partial_ws, void* stream);
int spo_ma_clip_adam(float* theta, const float* grad, float* adam_m, float* adam_v, int64_t n, int64_t adam_step_host,
                     float lr, float adam_eps, float weight_decay, float max_grad_norm, int use_max_grad_norm,
                     float* grad_norm_out, double* partial_ws, void* stream);

/* MACPO's trust-region step without host round trips (csrc/multi_agent.hip), the form the data-parallel trainer runs
 * (safepo/multi_agent/macpo.py, MACPO_Trainer with world_size > 1 or macpo_sharded_form).
 *
 * spo_ma_trpo_linesearch_sums replaces reference safepo/multi_agent/macpo.py:329-366 up to the accept test (evaluate_actions'
 * log-probabilities, ratio = prod_d exp(logp_d - old_logp_d), the two surrogate means and the mean of kl_divergence,
 * macpo.py:153-166): one row pass over mean / act / old_logp / mu_old [rows, act_dim], adv / cost_adv / factor [rows],
 * log_std / std_old [act_dim] with std = std_y_coef * sigmoid(log_std / std_x_coef) and the per-dimension log-probability of
 * spo_ma_log_probs.  sums4_out (device, fp64) = {sum ratio*factor*adv, sum ratio*factor*cost_adv, sum KL_row, sum ratio}:
 * ROW SUMS of this rank, so a data-parallel caller all-reduces the four doubles and divides by the global row count;
 * ratio_out_or_null: float[rows], the per-row ratio.  Reduced in a fixed order (per-block fp64 partials in partial_ws, then one
 * workgroup per sum; no atomics): the same rows give the same bits on every call and every rank.
 * partial_ws: double[SPO_MA_LS_WS_DOUBLES].  1 <= act_dim <= SPO_MAX_ACT, rows >= 1.
 *
 * spo_ma_cg_init / spo_ma_cg_update replace the body of conjugate_gradient (macpo.py:168-185) around the Fisher-vector product:
 * x, r, p: float[n] and state4 = {rdotr, done, last alpha, last beta} stay on the device.
 *   init:    x = 0, r = p = b, rdotr = b.b, done = 0
 *   update:  alpha = rdotr / (p.avp + 1e-8); x += alpha p; r -= alpha avp; new = r.r; p = r + (new / rdotr) p; rdotr = new;
 *            done = new < residual_tol.  With done set an update changes nothing, so nsteps enqueued updates give what the
 *            reference's `break` gives and no host read is needed inside a solve.
 * Dot products accumulate in fp64 and round once to fp32; the scalar recurrences are fp32 in the reference's order.  One launch
 * per update up to 16384 elements, two beyond (any n); fixed-order reductions.  ws: double[SPO_MA_CG_WS_DOUBLES], owned by the
 * solve between init and its last update. */
#define SPO_MA_LS_WS_DOUBLES 4096
#define SPO_MA_CG_WS_DOUBLES 520
int spo_ma_trpo_linesearch_sums(const float* mean, const float* log_std, float std_x_coef, float std_y_coef, const float* act,
                                const float* old_logp, const float* adv, const float* cost_adv, const float* factor,
                                const float* mu_old, const float* std_old, int64_t rows, int act_dim, double* sums4_out,
                                float* ratio_out_or_null, double* partial_ws, void* stream);
int spo_ma_cg_init(const float* b, float* x, float* r, float* p, float* state4, double* ws, int64_t n, void* stream);
int spo_ma_cg_update(const float* avp, float* x, float* r, float* p, float* state4, double* ws, int64_t n, float residual_tol,
                     void* stream);

/* Test hook for the plain products of csrc/gemm_f32.hip: y[B,N] = x[B,K] w[N,K]^T (mode 0) or y[B,K] = x[B,N] w[N,K]
 * (mode 1) through the hand-written fp32 MFMA kernel, what spo_ma_forward / backward / jvp and the wide path run.
 * use_rocblas must be 0: the rocBLAS comparator it once selected was removed (nonzero: -1, spo_last_error names the removal). */
int spo_debug_ma_gemm(int use_rocblas, int mode, const float* x, const float* w, float* y, int64_t B, int K, int N, void* stream);

/* ---- wide single-agent networks (csrc/wide.hip): ActorVCritic(obs_dim, act_dim, hidden_sizes) for any hidden_sizes (reference
 * safepo/common/model.py:30-48,131; isaac_gym_specific_cfg = [1024, 1024, 512], safepo/single_agent/ppo_lag.py:54-65).
 * A network is n_layers Linear layers with tanh between them; dims[0] = input width, dims[n_layers] = output width.
 * Flat layout of one network: for each layer W [out, in] row-major, then b [out] (nn.Sequential.parameters() order).
 * spo_mlp_forward leaves every layer's activations in ws (float[spo_mlp_workspace_floats]); the output is the LAST
 * rows * dims[n_layers] floats of ws.  spo_mlp_backward takes d(loss)/d(output) and writes the network's flat gradient;
 * scratch: float[spo_mlp_backward_scratch_floats].
 * spo_wide_ppo_loss (ppo_lag.py:306-323): MSE of both critics (WITHOUT their L2 terms), the clipped surrogate, their output
 * gradients and d(loss)/d(log_std); partial_ws: double[>= 256 * (3 + SPO_WIDE_MAX_ACT) + 512].
 * spo_wide_clip_adam (ppo_lag.py:310-329): adds the critics' L2 gradient 2 * l2_coef * p (cfg->use_critic_norm) and the value
 * coefficient (cfg->use_value_coefficient) to `grad` in place, adds l2_coef * sum p^2 to losses3_inout[0..1], clips the joint
 * norm over all n_params to cfg->max_grad_norm and takes one Adam step with cfg->lr_critic for [0, actor_begin) and
 * cfg->lr_actor beyond.  scalars4_out = {clip coefficient, L2 term of the reward critic, of the cost critic, ||g||};
 * partial_ws: double[>= 3 * 1024]. */
#define SPO_MLP_MAX_LAYERS 5
typedef struct spo_mlp_net {
  int32_t n_layers;
  int32_t dims[SPO_MLP_MAX_LAYERS + 1];
} spo_mlp_net;
int64_t spo_mlp_param_count(const spo_mlp_net* net);
int64_t spo_mlp_workspace_floats(const spo_mlp_net* net, int64_t rows);
int64_t spo_mlp_backward_scratch_floats(const spo_mlp_net* net, int64_t rows);
int spo_mlp_forward(const float* theta, const spo_mlp_net* net, const float* x, int64_t rows, float* ws, void* stream);
int spo_mlp_backward(const float* theta, const spo_mlp_net* net, const float* x, int64_t rows, const float* ws,
                     const float* d_out, float* grad, float* scratch, void* stream);
/* Up to 128 rows (and layer widths whose row images fit LDS: csrc/mlp_small.hip) spo_mlp_forward / spo_mlp_backward run the
 * WHOLE network in one launch each (one workgroup, weights staged through LDS layer by layer) instead of a GEMM launch per
 * layer: the reference's default minibatch of 64 is launch-latency territory.  SPO_MLP_SMALL=0 keeps the per-layer launches.
 * The _multi forms take `count` (<= 4) networks on the same number of rows -- the networks of a minibatch step -- and put them
 * into ONE launch (one workgroup per network) when all of them fit, else call the single-network entry point per network. */
int spo_mlp_forward_multi(int count, const float* const* thetas, const spo_mlp_net* const* nets, const float* const* xs,
                          int64_t rows, float* const* wss, void* stream);
int spo_mlp_backward_multi(int count, const float* const* thetas, const spo_mlp_net* const* nets, const float* const* xs,
                           int64_t rows, const float* const* wss, const float* const* d_outs, float* const* grads,
                           float* const* scratches, void* stream);
/* Round 6: the forward / loss / backward of a whole PPO-Lagrangian minibatch (ppo_lag.py:298-324: DataLoader batch, both critics'
 * MSE, the clipped surrogate, loss.backward()) for ANY hidden_sizes at up to 256 rows in ONE launch, split over the rows
 * (csrc/mlp_rows.hip): networks x ceil(rows / 16) workgroups, each carrying 16 rows of one network through every layer both ways
 * with the activations in LDS and the weights read as MFMA operands straight from global memory; the rows are
 * idx[*cursor_dev + i] (cursor_dev NULL: idx[i]; idx NULL: the rows themselves) of the FULL arrays obs [M, obs_dim], act, logp_old,
 * targets, adv -- no gather launch.  theta = [reward critic | cost critic | log_std | actor] (the ActorVCritic layout), `critic` /
 * `actor` describe the networks; actor NULL: the two critics only (the critic fit of cpo.py:541-556).  Every workgroup writes its
 * row group's partial gradient (theta's layout, WITHOUT the L2 terms) and loss sums into parts (float[spo_wide_grad_rows_part_floats]);
 * spo_wide_reduce_parts adds the groups in fixed order into grad[n_params] and forms losses_out[0 .. n_losses) = {MSE reward critic,
 * MSE cost critic, clipped surrogate}: what spo_gather_rows + spo_mlp_forward_multi + spo_wide_ppo_loss + spo_mlp_backward_multi
 * leave in `grad` / losses3, and where the data-parallel all-reduce and spo_wide_clip_adam take over.  SPO_WIDE_ROWS=0 makes
 * spo_wide_grad_rows_supported return 0 (callers then keep the launch-per-network path). */
int spo_wide_grad_rows_supported(const spo_mlp_net* critic, const spo_mlp_net* actor, int64_t rows);
int64_t spo_wide_grad_rows_part_floats(int64_t n_params, int64_t rows);
int spo_wide_ppo_grad_rows(const float* theta, const spo_mlp_net* critic, const spo_mlp_net* actor, const float* obs,
                           const float* act, const float* logp_old, const float* target_r, const float* target_c, const float* adv,
                           const int64_t* idx, const int64_t* cursor_dev, int64_t rows, float clip, float* parts, void* stream);
int spo_wide_reduce_parts(const float* parts, int64_t rows, int64_t n_params, int n_losses, float* grad, float* losses_out,
                          void* stream);
/* spo_wide_reduce_parts + spo_wide_clip_adam_dev_log (all parameters in the norm and in the Adam range: ppo_lag.py:310-329) in TWO
 * launches instead of four: the group sum rides in the pass that adds the L2 gradient and forms the norm partials (its first
 * workgroup also advances the optimiser clocks and the cursor); every workgroup of the Adam pass forms the clip coefficient from the
 * partials itself, the first one logs the losses.  Element for element the arithmetic of the four launches.  One GPU (a
 * data-parallel step all-reduces between the sum and the clip). */
int spo_wide_rows_clip_adam_dev_log(float* parts, int64_t rows, float* theta, float* grad, float* adam_m, float* adam_v,
                                    int64_t n_params, int64_t reward_critic_end, int64_t cost_critic_end, int64_t actor_begin,
                                    const spo_ppo_cfg* cfg, double* pow4_dev, float* losses3_out, float* scalars4_out,
                                    double* partial_ws, int partial_capacity, float* loss_log_dev, int64_t* cursor_dev,
                                    int64_t cursor_step, void* stream);
/* Seed-batched form of the fused step above (spo_wide_ppo_grad_rows + spo_wide_rows_clip_adam_dev_log): S independent runs of ONE
 * shape (critic, actor, rows) in the same three launches, run r on the grid slice blockIdx.y == r.  Each run's blocks read the
 * arguments its stand-alone launches would receive from a device table and run the same kernel bodies on the same blockIdx.x /
 * gridDim.x, so per run the step is bit for bit its own stand-alone sequence (partial sums and their order included).  No workgroup
 * of these kernels waits for another: there is no exchange, no placement census, no per-XCD budget and no timeout path -- the cap
 * of 32 runs bounds the table only.  A run with active == 0 is skipped: its blocks return before they touch memory, nothing of it
 * is read or written, and its pointers may be NULL.
 * spo_wide_rows_replica -- one run's pointers: everything the two stand-alone entries take.  perm / cursor_dev / loss_log_dev are a
 *   PermWindow's arrays (the rows perm[*cursor_dev .. + rows); the step stores its losses at loss_log_dev[3 * (*cursor_dev /
 *   cursor_step)] and moves the cursor on; loss_log_dev may be NULL), pow4_dev the run's device clocks and learning rates
 *   (double[6], spo_wide_clip_adam_dev), partial_ws double[partial_capacity >= 3 * min(ceil(n_params / 256), 1024)].  cfg: clip, the
 *   L2 / value-coefficient options, max_grad_norm, betas, eps (learning rates: pow4_dev[4..5] where >= 0).
 * spo_wide_rows_multi_supported -- 1 where spo_wide_grad_rows_supported(critic, actor, rows) holds with an actor and
 *   1 <= n_replicas <= SPO_WIDE_ROWS_MAX_REPLICAS.  Host only.
 * spo_wide_rows_multi_table_bytes -- bytes of the device table for n_replicas runs (-1 outside the cap).
 * spo_wide_rows_multi_upload -- validates reps_host[n_replicas] (a HOST array), fills every active run's kernel arguments through the
 *   code the stand-alone entries use and copies the table to table_dev (stream-ordered; returns when the copy is done).  Refused
 *   before any HIP call, in this order: a null table, n_replicas outside the cap, an unsupported shape, a null pointer of an active
 *   run, two active runs sharing theta, parts or cursor_dev, parameter ranges out of order, a partial workspace too small,
 *   cursor_step <= 0; then a stream under capture.
 * spo_wide_rows_step_multi -- the three launches for all runs of an uploaded table: no allocation, no copy, no host read, so the
 *   call can be captured into a HIP graph and replayed (the table is read at every replay: upload a new one between replays to
 *   change the active flags). */
#define SPO_WIDE_ROWS_MAX_REPLICAS 32
typedef struct {
  float *theta, *adam_m, *adam_v;          /* the run's own parameters and moments */
  float *grad, *parts;                     /* float[n_params]; float[spo_wide_grad_rows_part_floats(n_params, rows)] */
  const float *obs, *act, *logp_old, *target_r, *target_c, *adv;   /* the FULL arrays of the run's buffer */
  const int64_t* perm;                     /* the run's shuffle (device) */
  int64_t* cursor_dev;                     /* position in perm, advanced by cursor_step per step */
  double* pow4_dev;                        /* double[6]: beta powers of both optimiser clocks, the two learning rates */
  float *losses3_out, *scalars4_out;       /* the step's losses; {clip coefficient, L2 terms, gradient norm} */
  double* partial_ws;
  int partial_capacity;
  float* loss_log_dev;                     /* [steps of a pass][3], or NULL */
  spo_ppo_cfg cfg;
  int active;
} spo_wide_rows_replica;
int spo_wide_rows_multi_supported(const spo_mlp_net* critic, const spo_mlp_net* actor, int64_t rows, int n_replicas);
int64_t spo_wide_rows_multi_table_bytes(int n_replicas);
int spo_wide_rows_multi_upload(void* table_dev, const spo_wide_rows_replica* reps_host, int n_replicas, const spo_mlp_net* critic,
                               const spo_mlp_net* actor, int64_t rows, int64_t cursor_step, void* stream);
int spo_wide_rows_step_multi(const void* table_dev, int n_replicas, const spo_mlp_net* critic, const spo_mlp_net* actor, int64_t rows,
                             void* stream);
/* The KL-penalty loss of FOCOPS (focops.py:326-347) and of CUP's actor-only second stage (cup.py:370-386) on the row groups of
 * spo_wide_ppo_grad_rows: same rows (idx / cursor_dev / rows as there), same theta layout, one launch.  The loss needs
 * F = mean_i(ind_i), ind_i = [KL_i <= kl_bound], before its cotangent; its gradient is linear in F, g_actor = g_KL + F * g_PG with
 * both parts sums over rows, so the actor runs in TWO kinds of workgroup per row group: one backpropagates ind_i d(KL_i)/d(mean) / rows
 * (d(log_std) term ind_i (vrat - 1) / rows), the other -(pg_coef / rows) d(ratio_i adv_i)/d(mean) with F taken as 1; the critics'
 * workgroups (absent with actor_only) are those of the PPO launch.  Per-row arithmetic: spo_wide_kl_penalty_split's.
 * old_mean [M, act_dim] is read through the index window like act, old_std is [act_dim]; kl_bound = +inf (CUP) gives ind_i = 1.
 * spo_wide_kl_penalty_grad_rows_supported -- 1 when spo_wide_grad_rows_supported holds AND the launch's own LDS need (the old
 *   distribution of the 16 rows sits behind the actor's images) fits one CU; 0 with SPO_WIDE_ROWS=0.
 * spo_wide_kl_penalty_rows_part_floats -- floats of `parts` (actor_begin = the offset of log_std, 2 * critic parameters); the tail
 *   behind the row groups' parts holds n_params + SPO_KLPEN_SUMS floats a caller may hand to the reduce as pg_grad / sums.
 * spo_wide_kl_penalty_reduce_parts -- the groups added in group order (deterministic, no atomics):
 *   combine == 0 (data-parallel): grad[lo, n_params) = the critics' data gradients (no L2 term) and g_KL in the actor's block,
 *     lo = actor_begin with actor_only, else 0; pg_grad[actor_begin, n_params) (indexed like grad) = g_PG with F = 1;
 *     sums[SPO_KLPEN_SUMS] = {0, 0, count of ind, sum ind*KL, sum ratio*adv, rows} (spo_wide_kl_penalty_split's layout);
 *     losses_out[0..1] = the critics' data losses (not with actor_only).  Then the all-reduce and spo_wide_kl_penalty_combine.
 *   combine != 0 (one GPU): additionally the actor's block of grad becomes g_KL + F * g_PG, F = sums[2] / sums[5], and
 *     losses_out[2] = (sums[3] - pg_coef * F * sums[4]) / sums[5] -- bit for bit what combine == 0 followed by
 *     spo_wide_kl_penalty_combine(grad_scale = 1) gives.  Then spo_wide_clip_adam_ex / spo_wide_clip_adam_dev_log.
 * Both launch entry points refuse null pointers, shapes outside ..._supported and rows outside 1..256 before any launch. */
int spo_wide_kl_penalty_grad_rows_supported(const spo_mlp_net* critic, const spo_mlp_net* actor, int64_t rows);
int64_t spo_wide_kl_penalty_rows_part_floats(int64_t n_params, int64_t actor_begin, int64_t rows);
int spo_wide_kl_penalty_grad_rows(const float* theta, const spo_mlp_net* critic, const spo_mlp_net* actor, const float* obs,
                                  const float* act, const float* logp_old, const float* target_r, const float* target_c,
                                  const float* adv, const float* old_mean, const float* old_std, const int64_t* idx,
                                  const int64_t* cursor_dev, int64_t rows, float kl_bound, float pg_coef, int actor_only,
                                  float* parts, void* stream);
int spo_wide_kl_penalty_reduce_parts(const float* parts, int64_t rows, int64_t n_params, int64_t actor_begin, int actor_only,
                                     int combine, float pg_coef, float* grad, float* pg_grad, float* sums, float* losses_out,
                                     void* stream);
/* Seed-batched form of the row-group step of FOCOPS and CUP: S independent runs of ONE shape (critic, actor, rows) in the
 * stand-alone step's FIVE launches, run r on the grid slice blockIdx.y == r of each (the coefficient launch: one wave per run, grid
 * (1, S)).  actor_loss / actor_only are launch-wide, as in spo_update_iter_ex_multi, and select the step's kind:
 *   SPO_ACTOR_LOSS_KL_PENALTY, actor_only = 0 (FOCOPS):  spo_wide_kl_penalty_grad_rows, spo_wide_kl_penalty_reduce_parts(combine = 1),
 *     spo_wide_clip_adam_dev_log(adam range [0, n_params), norm_begin 0, losses3_inout = log_src = losses3_out);
 *   SPO_ACTOR_LOSS_KL_PENALTY, actor_only = 1 (CUP's second stage): the same two with actor_only = 1, then
 *     spo_wide_clip_adam_dev_log(adam range [actor_begin, n_params), norm_begin = actor_begin, losses3_inout = NULL): the norm over the
 *     actor's range, the actor's clock only; the critics' parameters, moments and clocks are not touched;
 *   SPO_ACTOR_LOSS_CLIP, actor_only = 0 (CUP's first stage, the clipped surrogate on `adv`): spo_wide_ppo_grad_rows,
 *     spo_wide_reduce_parts(3 losses), spo_wide_clip_adam_dev_log as for FOCOPS.
 * Each run's blocks read the arguments its stand-alone launches would receive from a device table and run the same kernel bodies on
 * the same blockIdx.x / gridDim.x, so per run the step is bit for bit its own stand-alone sequence.  No workgroup waits for
 * another: no exchange, no placement census, no per-XCD budget, no timeout path -- the cap of SPO_WIDE_ROWS_MAX_REPLICAS runs bounds
 * the table only.  A run with active == 0 is skipped: its blocks return before they touch memory; its pointers may be NULL.
 * spo_wide_rows_ex_replica -- spo_wide_rows_replica's fields plus the old distribution and the loss options of the run.  parts:
 *   float[spo_wide_kl_penalty_rows_part_floats(n_params, actor_begin, rows)] with the KL-penalty loss (the reduce's pg_grad / sums
 *   are the buffer's tail behind the row groups), float[spo_wide_grad_rows_part_floats(n_params, rows)] with the clipped surrogate.
 *   losses3_out is also the row the step logs (log_src); with actor_only only losses3_out[2] is written.  target_r / target_c may be
 *   NULL with actor_only, old_mean / old_std with the clipped surrogate (kl_bound / pg_coef are then unused).
 * spo_wide_rows_ex_multi_supported -- 1 where the kind exists (actor_only needs the KL-penalty loss), 1 <= n_replicas <=
 *   SPO_WIDE_ROWS_MAX_REPLICAS and spo_wide_kl_penalty_grad_rows_supported (KL penalty) / spo_wide_grad_rows_supported (clipped
 *   surrogate) holds with an actor.  Host only.
 * spo_wide_rows_ex_multi_table_bytes -- bytes of the device table for n_replicas runs (-1 outside the cap).
 * spo_wide_rows_ex_multi_upload -- validates reps_host[n_replicas] (a HOST array), fills every active run's kernel arguments through
 *   the code the stand-alone entries use and copies the table to table_dev (stream-ordered; returns when the copy is done).  Refused
 *   before any HIP call, in this order: a null table, n_replicas outside the cap, an unknown actor_loss, actor_only with the clipped
 *   surrogate, an unsupported shape, a null pointer of an active run, two active runs sharing theta, parts or cursor_dev,
 *   cursor_step <= 0, then per active run parameter ranges out of order, a partial workspace too small, betas outside [0, 1); then a
 *   stream under capture.
 * spo_wide_rows_ex_step_multi -- the five launches for all runs of an uploaded table (same n_replicas / shape / kind as the upload):
 *   no allocation, no copy, no host read, so the call can be captured into a HIP graph and replayed. */
typedef struct {
  float *theta, *adam_m, *adam_v;          /* the run's own parameters and moments */
  float *grad, *parts;                     /* float[n_params]; the row groups' parts (see above) */
  const float *obs, *act, *logp_old, *target_r, *target_c, *adv;   /* the FULL arrays of the run's buffer */
  const int64_t* perm;                     /* the run's shuffle (device) */
  int64_t* cursor_dev;                     /* position in perm, advanced by cursor_step per step */
  double* pow4_dev;                        /* double[6]: beta powers of both optimiser clocks, the two learning rates */
  float *losses3_out, *scalars4_out;       /* the step's losses; {clip coefficient, L2 terms, gradient norm} */
  double* partial_ws;
  int partial_capacity;
  float* loss_log_dev;                     /* [steps of a pass][3], or NULL */
  spo_ppo_cfg cfg;
  int active;
  const float *old_mean, *old_std;         /* old_mean [M, act_dim] (read through perm), old_std [act_dim] */
  float kl_bound, pg_coef;
} spo_wide_rows_ex_replica;
int spo_wide_rows_ex_multi_supported(const spo_mlp_net* critic, const spo_mlp_net* actor, int64_t rows, int actor_loss, int actor_only,
                                     int n_replicas);
int64_t spo_wide_rows_ex_multi_table_bytes(int n_replicas);
int spo_wide_rows_ex_multi_upload(void* table_dev, const spo_wide_rows_ex_replica* reps_host, int n_replicas, const spo_mlp_net* critic,
                                  const spo_mlp_net* actor, int64_t rows, int64_t cursor_step, int actor_loss, int actor_only,
                                  void* stream);
int spo_wide_rows_ex_step_multi(const void* table_dev, int n_replicas, const spo_mlp_net* critic, const spo_mlp_net* actor, int64_t rows,
                                int actor_loss, int actor_only, void* stream);
/* dsts[k][i, :] = srcs[k][idx[i], :] for k < count (<= SPO_GATHER_MAX) row-major arrays of widths[k] floats per row: the
 * minibatch gather of a step (the reference's DataLoader, ppo_lag.py:298-305) in one launch. */
#define SPO_GATHER_MAX 8
int spo_gather_rows(int count, const float* const* srcs, const int* widths, float* const* dsts, const int64_t* idx, int64_t n,
                    void* stream);
/* The same on the window idx[*cursor_dev .. *cursor_dev + n) of a longer index vector (cursor_dev: device int64, may be NULL =
 * 0): a launch captured into a HIP graph then walks a permutation, one minibatch per replay, with spo_wide_clip_adam_dev_log
 * advancing the cursor. */
int spo_gather_rows_at(int count, const float* const* srcs, const int* widths, float* const* dsts, const int64_t* idx,
                       const int64_t* cursor_dev, int64_t n, void* stream);
/* rsample + log-prob of a diagonal Gaussian (model.py:149-170; eps == NULL: deterministic), and the row sum of
 * KL(N(mean_old, exp(log_std_old)) || N(mean_new, exp(log_std_new))).sum(-1) (ppo_lag.py:338-345) added to (accumulate != 0) or
 * stored into *sum_inout -- the full batch is evaluated in row chunks. */
int spo_gauss_sample(const float* mean, const float* log_std, const float* eps, float* act_out, float* logp_out, int64_t rows,
                     int act_dim, void* stream);
int spo_gauss_kl_sum(const float* mean_old, const float* log_std_old, const float* mean_new, const float* log_std_new,
                     int64_t rows, int act_dim, double* partial_ws, int partial_capacity, double* sum_inout, int accumulate,
                     void* stream);
int spo_wide_ppo_loss(const float* v_r, const float* v_c, const float* mean, const float* log_std, const float* act,
                      const float* logp_old, const float* adv, const float* tgt_r, const float* tgt_c, int64_t rows,
                      int act_dim, float clip, float* d_vr, float* d_vc, float* d_mean, float* d_log_std, float* losses3,
                      double* partial_ws, int partial_capacity, void* stream);
int spo_wide_clip_adam(float* theta, float* grad, float* adam_m, float* adam_v, int64_t n_params, int64_t reward_critic_end,
                       int64_t cost_critic_end, int64_t actor_begin, const spo_ppo_cfg* cfg, int64_t adam_step_host,
                       float* losses3_inout, float* scalars4_out, double* partial_ws, int partial_capacity, void* stream);


/* ---- round 4 (csrc/wide.hip): the wide path as the fallback for any (obs_dim, act_dim, hidden_sizes) and every single-agent script.  The
 * reference's ActorVCritic takes any dims (safepo/common/model.py:131) and its default sweep (safepo/single_agent/benchmark.py:5-44)
 * pairs cpo / pcpo / rcpo / trpo_lag / focops / cup / ppo_lag / cppo_pid with tasks of 72-88 observations (Car, Doggo, Racecar)
 * and with HumanoidVelocity (376 observations, 17 actions).  act_dim <= SPO_WIDE_MAX_ACT.
 * spo_wide_actor_loss -- actor loss of rows [0, rows) of a (possibly chunked) batch of rows_total rows and d(loss)/d(mean):
 *   mode 0  clipped PPO surrogate -mean(min(ratio*adv, clamp(ratio, 1-p0, 1+p0)*adv))          (ppo_lag.py:316-319)
 *   mode 1  p0 * mean(ratio*adv), p0 = sign: the CPO / TRPO surrogates                          (cpo.py:356-381)
 *   mode 2  KL-penalty loss of FOCOPS / CUP's second stage, p0 = kl_bound, p1 = pg_coef (see spo_update_iter_ex); needs
 *           old_mean[rows, act_dim], old_std[act_dim]; minibatch only (rows == rows_total, accumulate == 0).
 *   sums_inout double[2 + act_dim] = {sum of the loss terms, sum of the KL indicators, d(loss)/d(log_std)[act_dim]}, added to
 *   (accumulate != 0) or overwritten; loss_out / d_log_std_out (optional, float) receive the finished loss and d(log_std).
 *   partial_ws: double[>= 256 * (2 + SPO_WIDE_MAX_ACT)].
 * spo_wide_critic_loss -- MSE of both critics and their output gradients (critic fit, cpo.py:541-556); losses2[0..1];
 *   partial_ws: double[>= 512].
 * spo_mlp_jvp -- forward-mode tangent dout[rows, out] = d(out)/d(theta) . tangent (tangent laid out like the network's theta)
 *   at the activations spo_mlp_forward left in ws; with spo_wide_fvp_cotangent (d_mean = (J t) / sigma^2 / (rows_total * act_dim))
 *   and spo_mlp_backward this is one chunk of the Fisher-vector product J^T diag(1/sigma^2) J t / (M * A) of cpo.py:132-157
 *   (the reference differentiates the KL twice).  scratch: float[spo_mlp_jvp_scratch_floats].
 * spo_wide_linesearch_sums -- sums3 = {sum ratio*adv_a, sum ratio*adv_b, sum_{rows,dims} KL(old || new)} (cpo.py:473-491) of
 *   one row chunk, added to (accumulate != 0) or stored into sums3_inout.  partial_ws: double[3 * blocks], blocks <= 512.
 * spo_wide_clip_adam_ex -- spo_wide_clip_adam with (i) the joint norm taken over [norm_begin, n_params) (0: all parameters;
 *   actor_begin - act_dim: CUP's actor-only clip, cup.py:385), (ii) Adam applied to [adam_begin, adam_end) only, the
 *   critics' optimisers at adam_step_critics_host and the actor's at adam_step_actor_host, (iii) scale_rest != 0: gradients
 *   outside the Adam range multiplied by the clip coefficient in place -- what clip_grad_norm_ over ALL policy parameters does to
 *   the actor's stale gradient during the critic fit (cpo.py:557).  The critics' L2 term / value coefficient are applied when
 *   norm_begin == 0 (as in spo_wide_clip_adam). */
int spo_wide_actor_loss(int mode, const float* mean, const float* log_std, const float* act, const float* logp_old,
                        const float* adv, const float* old_mean, const float* old_std, int64_t rows, int64_t rows_total,
                        int act_dim, float p0, float p1, float* d_mean, double* sums_inout, int accumulate, float* loss_out,
                        float* d_log_std_out, double* partial_ws, int partial_capacity, void* stream);
/* Data-parallel FOCOPS / CUP on the wide path (the split form of spo_kl_penalty_grad / spo_clip_adam_ex for shapes outside the
 * persistent kernels; replaces focops.py:326-347 and cup.py:370-386 under torchrun).  The KL-penalty loss of spo_wide_actor_loss
 * mode 2 needs F = mean_i(ind_i) of the minibatch before its cotangent; the gradient is linear in F, g = g_KL + F * g_PG, so:
 * spo_wide_kl_penalty_split -- one unchunked local minibatch of `rows` rows: d_mean_kl[rows, act_dim] = ind_i d(KL_i)/d(mean) / rows,
 *   d_mean_pg[rows, act_dim] = -(pg_coef / rows) d(ratio_i adv_i)/d(mean) (F taken as 1), the two parts of d(log_std) into
 *   d_log_std_kl[act_dim] / d_log_std_pg[act_dim], and sums float[SPO_KLPEN_SUMS] = {0, 0, count of ind, sum ind*KL,
 *   sum ratio*adv, rows} (spo_kl_penalty_grad's layout).  partial_ws: double[>= 256 * (3 + 2 * SPO_WIDE_MAX_ACT)].  The caller
 *   backpropagates both cotangents (the PG one into a buffer of its own) and all-reduces gradients + sums.
 * spo_wide_kl_penalty_combine -- after the all-reduce: grad[begin, n_params) *= grad_scale, with grad[i] += F * pg_grad[i] for
 *   i >= actor_begin first (pg_grad indexed like grad), F = sums[2] / sums[5]; loss_out (optional) = the global minibatch's
 *   actor loss (sums[3] - pg_coef * F * sums[4]) / sums[5].  Then spo_wide_clip_adam_ex (which adds the critics' L2 term). */
int spo_wide_kl_penalty_split(const float* mean, const float* log_std, const float* act, const float* logp_old, const float* adv,
                              const float* old_mean, const float* old_std, int64_t rows, int act_dim, float kl_bound, float pg_coef,
                              float* d_mean_kl, float* d_mean_pg, float* d_log_std_kl, float* d_log_std_pg, float* sums,
                              double* partial_ws, int partial_capacity, void* stream);
int spo_wide_kl_penalty_combine(float* grad, const float* pg_grad, const float* sums, int64_t n_params, int64_t begin,
                                int64_t actor_begin, float grad_scale, float pg_coef, float* loss_out, void* stream);
int spo_wide_critic_loss(const float* v_r, const float* v_c, const float* tgt_r, const float* tgt_c, int64_t rows, float* d_vr,
                         float* d_vc, float* losses2, double* partial_ws, int partial_capacity, void* stream);
int64_t spo_mlp_jvp_scratch_floats(const spo_mlp_net* net, int64_t rows);
int spo_mlp_jvp(const float* theta, const spo_mlp_net* net, const float* tangent, const float* x, int64_t rows, const float* ws,
                float* dout, float* scratch, void* stream);
int spo_wide_fvp_cotangent(const float* jv, const float* log_std, int64_t rows, int64_t rows_total, int act_dim, float* d_mean,
                           void* stream);
int spo_wide_linesearch_sums(const float* mean_new, const float* log_std_new, const float* act, const float* logp_old,
                             const float* adv_a, const float* adv_b, const float* mean_old, const float* log_std_old, int64_t rows,
                             int act_dim, double* partial_ws, int partial_capacity, double* sums3_inout, int accumulate,
                             void* stream);
/* spo_wide_clip_adam_dev -- spo_wide_clip_adam_ex with the optimiser clocks on the DEVICE: pow4_dev = double[6] = {beta1^t, beta2^t of
 * the critics' optimisers, beta1^t, beta2^t of the actor's} before this step, then {lr_actor, lr_critic} (each: >= 0 overrides the
 * cfg's value, so a schedule does not change a captured launch's arguments; negative: the cfg's -- ABI 2); the clocks of the optimisers inside the Adam range
 * advance on the device.  No argument changes from one minibatch step to the next, so the launch sequence of a step (gathers,
 * spo_mlp_forward / backward, loss kernels, this) can be captured once as a HIP graph and replayed: the wide path at the reference's
 * default batch of 64 is launch-bound (~70 launches per step).  The caller keeps pow4_dev in step with its host-side step counts. */
int spo_wide_clip_adam_dev(float* theta, float* grad, float* adam_m, float* adam_v, int64_t n_params, int64_t reward_critic_end,
                           int64_t cost_critic_end, int64_t actor_begin, const spo_ppo_cfg* cfg, double* pow4_dev, int64_t adam_begin,
                           int64_t adam_end, int64_t norm_begin, int scale_rest, float* losses3_inout, float* scalars4_out,
                           double* partial_ws, int partial_capacity, void* stream);
/* spo_wide_clip_adam_dev that also (cursor_dev != NULL) stores the step's three losses log_src_dev[0..2] (after the L2 terms were
 * added) at loss_log_dev[3 * (*cursor_dev / cursor_step)] and advances *cursor_dev by cursor_step: together with
 * spo_gather_rows_at a replayed minibatch step takes no host copy in (indices) or out (losses). */
int spo_wide_clip_adam_dev_log(float* theta, float* grad, float* adam_m, float* adam_v, int64_t n_params, int64_t reward_critic_end,
                               int64_t cost_critic_end, int64_t actor_begin, const spo_ppo_cfg* cfg, double* pow4_dev, int64_t adam_begin,
                               int64_t adam_end, int64_t norm_begin, int scale_rest, float* losses3_inout, float* scalars4_out,
                               double* partial_ws, int partial_capacity, float* loss_log_dev, const float* log_src_dev,
                               int64_t* cursor_dev, int64_t cursor_step, void* stream);
int spo_wide_clip_adam_ex(float* theta, float* grad, float* adam_m, float* adam_v, int64_t n_params, int64_t reward_critic_end,
                          int64_t cost_critic_end, int64_t actor_begin, const spo_ppo_cfg* cfg, int64_t adam_step_critics_host,
                          int64_t adam_step_actor_host, int64_t adam_begin, int64_t adam_end, int64_t norm_begin, int scale_rest,
                          float* losses3_inout, float* scalars4_out, double* partial_ws, int partial_capacity, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SAFEPO_HIP_H */
