// The host side of a replica-table launch, shared by the six seed-batched entry points (update_rs.hip:
// spo_ppo_lag_update_iter_multi, spo_critic_fit_iter_multi; update.hip: spo_update_iter_ex_multi, spo_critic_fit_iter_split_multi;
// update_ks.hip: spo_update_iter_ex_ks_multi, spo_critic_fit_iter_ks_multi).  Host-only: no device code lives here.
//   small helpers    stream_is_capturing, env_flag, block_map_query, upload_table
//   scratch blocks   alloc_block, free_block, ScratchForm: how the StreamTable users (stream_table.h) allocate, free and refuse
//   ReplicaPool      the scratch block + pinned table ring of one (device, stream), one instance per form
//   table checks     table_head, same_shape, distinct: the refusals every table type shares, worded with the entry's name
//   fill_run / fill_run_ex  the per-run fields of RsArgs / KsArgs / UpdArgs, one copy for the stand-alone entry and the table loop
// What an entry still writes itself is listed in DESIGN.md ("Adding a seed-batched form").
#pragma once
#include <cmath>
#include <cstdlib>
#include <type_traits>
#include "common.h"
#include "stream_table.h"
#include "update_rs.h"

namespace spo {

inline bool stream_is_capturing(hipStream_t st) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone;
}

// An on/off switch of the environment, read at every call: set, not empty and not starting with '0'.
inline int env_flag(const char* name) {
  const char* e = getenv(name);
  return (e && *e && *e != '0') ? 1 : 0;
}

// hip_check with the message "<call>(<what>): <error>"
inline int hip_check2(hipError_t e, const char* call, const char* what) {
  if (e == hipSuccess) return 0;
  snprintf(g_err, sizeof(g_err), "%s(%s): %s", call, what, hipGetErrorString(e));
  return (int)e;
}

// The spo_*_block_map exports: 1 and (*replica, *wg) where block `block` of a launch of n_replicas runs has work, else 0.
inline int block_map_query(int block, int n_replicas, int max_reps, int wgs, int* replica, int* wg) {
  if (n_replicas < 1 || n_replicas > max_reps || block < 0 || block >= rs_multi_grid(n_replicas, wgs)) return 0;
  int r = 0, w = 0;
  const bool work = rs_multi_map(block, n_replicas, wgs, &r, &w);
  if (work && replica) *replica = r;
  if (work && wg) *wg = w;
  return work ? 1 : 0;
}

// The table's copy to the device and the event behind it (the ring slot is rewritten only once that event has completed).
template <class Entry>
int upload_table(Entry* table_dev, const Entry* table_host, int n, hipEvent_t ev, hipStream_t st, const char* what) {
  if (int rc = hip_check2(hipMemcpyAsync(table_dev, table_host, (size_t)n * sizeof(Entry), hipMemcpyHostToDevice, st), "hipMemcpyAsync", what))
    return rc;
  return hip_check2(hipEventRecord(ev, st), "hipEventRecord", what);
}

// ---------------------------------------------------------------------------------------------------- scratch blocks
// hipMalloc of a scratch block: optionally zeroed, optionally with the device synchronised behind the memset.
inline int alloc_block(size_t bytes, bool zeroed, bool synced, const char* what, char** out) {
  void* p = nullptr;
  if (int rc = hip_check2(hipMalloc(&p, bytes), "hipMalloc", what)) return rc;
  int rc = zeroed ? hip_check2(hipMemset(p, 0, bytes), "hipMemset", what) : 0;
  if (!rc && zeroed && synced) rc = hip_check2(hipDeviceSynchronize(), "hipDeviceSynchronize", what);
  if (rc) { (void)hipFree(p); return rc; }
  *out = static_cast<char*>(p);
  return 0;
}

// hipFree of a block that spo_update_scratch_release lets go.  An error is recorded in the message buffer and otherwise ignored:
// the release goes on to the remaining blocks and still counts this one.
inline void free_block(void* p, const char* what) {
  if (p) (void)hip_check2(hipFree(p), "hipFree", what);
}

// What a single-run form says about its StreamTable (stream_table.h): the words of its two refusals and of its HIP errors, the
// size of a block and how a new one is prepared.
struct ScratchForm {
  const char* name;        // "<name>: more than ..." / "<name>: first launch on a stream under capture ..."
  const char* holds;       // "... pairs hold <holds> in this process ..."
  const char* made;        // "... (the <made> allocated on first use ..."
  const char* what;        // "hipMalloc(<what>)"
  size_t bytes; bool zeroed, synced;

  int refuse_full(int cap) const {
    return fail(-1, "%s: more than %d (device, stream) pairs hold %s in this process; call spo_update_scratch_release(stream) for "
                    "streams that are gone", name, cap, holds);
  }
  // the block of a pair's first launch: never under capture (allocation and memset would invalidate it)
  int first_use(hipStream_t st, char** out) const {
    if (stream_is_capturing(st))
      return fail(-1, "%s: first launch on a stream under capture (the %s allocated on first use: launch once outside the capture)",
                  name, made);
    return alloc_block(bytes, zeroed, synced, what, out);
  }
};

// ---------------------------------------------------------------------------------------------------- the replica-table pool
// One block per (device, stream) in a StreamTable, made at the pair's first launch (never under capture: the entries refuse that
// before) and kept until spo_update_scratch_release: `bytes` of device memory (0: none -- the split critic fit sizes its own),
// optionally zeroed with the device synchronised behind it, and a pinned host ring of RING argument tables of MAX_REPS entries,
// each with an event recorded behind its copy.  A launch takes the next ring slot and waits for that slot's event, so the host
// waits only when RING launches are already queued behind one another.  `Extra`: per-block state of one form (value-initialised
// with the block).  `before_free`: runs on a block that release() is about to free (counters that must outlive it).  The pool has
// no lock of its own: the caller holds the form's mutex around acquire() and keeps it until its table copy is enqueued, and
// around release().
struct NoExtra {};
template <class Entry, int MAX_REPS, int CAP, class Extra = NoExtra>
struct ReplicaPool {
  static constexpr int RING = 4;
  struct Block {
    int dev; void* stream; char* base;
    unsigned tag;                                    // tags of a launch: tag .. tag + nsteps + 1 (never reused within a block)
    Entry* tab_host; hipEvent_t ev[RING]; unsigned calls;
    Extra x;
  };
  struct Slot { Block* block; char* base; unsigned tag_base; Entry* tab_host; hipEvent_t ev; };

  size_t bytes; bool zeroed;
  const char* full_fmt;                              // the refusal at CAP pairs (one %d)
  const char* dev_what; const char* tab_what;        // names of the device block and of the table in HIP error messages
  void (*before_free)(Block&);
  StreamTable<Block, CAP> blocks = {};

  void free_block(Block& b) {
    spo::free_block(b.base, dev_what);
    if (b.tab_host) (void)hip_check2(hipHostFree(b.tab_host), "hipHostFree", tab_what);
    for (hipEvent_t ev : b.ev)
      if (ev) (void)hip_check2(hipEventDestroy(ev), "hipEventDestroy", tab_what);
    b = Block{};
  }

  int acquire(hipStream_t st, unsigned nsteps, Slot* out) {
    const int dev = current_device_slot();
    Block* b = blocks.find(dev, (void*)st);
    if (!b) {
      if (blocks.full()) return fail(-1, full_fmt, CAP);
      Block nb{};
      nb.dev = dev; nb.stream = (void*)st; nb.tag = 16u;
      if (bytes)
        if (int rc = alloc_block(bytes, zeroed, zeroed, dev_what, &nb.base)) return rc;
      void* p = nullptr;
      if (int rc = hip_check2(hipHostMalloc(&p, (size_t)RING * MAX_REPS * sizeof(Entry), hipHostMallocDefault), "hipHostMalloc", tab_what)) {
        free_block(nb); return rc;
      }
      nb.tab_host = static_cast<Entry*>(p);
      for (hipEvent_t& ev : nb.ev)
        if (int rc = hip_check2(hipEventCreateWithFlags(&ev, hipEventDisableTiming), "hipEventCreate", tab_what)) { free_block(nb); return rc; }
      b = blocks.add(nb);
    }
    const unsigned slot = b->calls++ % RING;
    *out = Slot{b, b->base, b->tag, b->tab_host + (size_t)slot * MAX_REPS, b->ev[slot]};
    b->tag += nsteps + 2u;                           // (wraps after 4e9 steps: a tag then meets words 2^32 steps old)
    // (an event that was never recorded is complete)
    return hip_check2(hipEventSynchronize(out->ev), "hipEventSynchronize", tab_what);
  }

  int release(int dev, void* stream_or_null, int all) {
    return blocks.release(dev, stream_or_null, all, [this](Block& b) {
      if (before_free) before_free(b);
      free_block(b);
    });
  }
};

// ---------------------------------------------------------------------------------------------------- table checks
// The refusals that spo_update_replica, spo_update_ex_replica and spo_critic_fit_replica tables share, worded with the entry's
// name.  One function per refusal, not one for the table: the entries interleave them differently with their own checks, and
// which refusal a malformed table meets first is part of each entry's behaviour (tests/test_seed_batch*_host.py).
template <class Rep>
int table_head(const char* name, const Rep* reps, int n_replicas, int max_reps) {
  SPO_REQUIRE(reps, "%s: null replica table", name);
  SPO_REQUIRE(n_replicas >= 1 && n_replicas <= max_reps, "%s: %d replicas outside [1, %d]", name, n_replicas, max_reps);
  return 0;
}

template <class Rep>
int same_shape(const char* name, const Rep* reps, int r) {
  const spo_ppo_cfg &c = reps[r].cfg, &c0 = reps[0].cfg;
  SPO_REQUIRE(c.obs_dim == c0.obs_dim && c.act_dim == c0.act_dim && c.batch == c0.batch,
              "%s: replica %d has obs_dim / act_dim / batch %d / %d / %d, replica 0 has %d / %d / %d", name, r, c.obs_dim, c.act_dim,
              c.batch, c0.obs_dim, c0.act_dim, c0.batch);
  return 0;
}

// no earlier run shares run r's theta or sync_ws -- or, in a critic-fit table, its stale_sq_io
template <class Rep>
int distinct(const char* name, const Rep* reps, int r) {
  for (int q = 0; q < r; ++q) {
    if constexpr (std::is_same<Rep, spo_critic_fit_replica>::value)
      SPO_REQUIRE(reps[q].theta != reps[r].theta && reps[q].sync_ws != reps[r].sync_ws && reps[q].stale_sq_io != reps[r].stale_sq_io,
                  "%s: replicas %d and %d share theta, sync_ws or stale_sq_io", name, q, r);
    else
      SPO_REQUIRE(reps[q].theta != reps[r].theta && reps[q].sync_ws != reps[r].sync_ws, "%s: replicas %d and %d share theta or sync_ws",
                  name, q, r);
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------------- argument fills
// The per-run fields that RsArgs, KsArgs and UpdArgs share, from one run's inputs: called by the stand-alone entry and by the
// table loop of its seed-batched form, so run r of a batched launch gets the stand-alone launch's argument values by construction.
// What differs between the two is set by the caller afterwards: scratch pointers, tag_base, force_safe, profile and staging
// fields, exchange regions.
template <class Args>
void fill_run(Args& a, float* theta, float* adam_m, float* adam_v, int64_t adam_step, const float* obs, const float* act,
              const float* logp_old, const float* target_r, const float* target_c, const float* adv, const int32_t* perm, int64_t M,
              const spo_ppo_cfg& cfg, int n_nets, int first_net, float* stale_io, float* losses, void* sync_ws) {
  a.theta = theta; a.adam_m = adam_m; a.adam_v = adam_v;
  a.obs = obs; a.act = act; a.logp_old = logp_old; a.tgt_r = target_r; a.tgt_c = target_c; a.adv = adv;
  a.perm = perm; a.M = M; a.cfg = cfg; a.losses = losses;
  a.err = reinterpret_cast<int*>(reinterpret_cast<char*>(sync_ws) + 64);
  a.pow_b1 = pow((double)cfg.beta1, (double)adam_step);
  a.pow_b2 = pow((double)cfg.beta2, (double)adam_step);
  a.n_nets = n_nets; a.first_net = first_net; a.stale_io = stale_io;
}

// ... and of the structs that also carry the actor's own optimiser clock and the KL-penalty loss (KsArgs, UpdArgs)
template <class Args>
void fill_run_ex(Args& a, float* theta, float* adam_m, float* adam_v, int64_t adam_step_critics, int64_t adam_step_actor, const float* obs,
                 const float* act, const float* logp_old, const float* target_r, const float* target_c, const float* adv,
                 const int32_t* perm, int64_t M, const spo_ppo_cfg& cfg, int n_nets, int first_net, float* stale_io, float* losses,
                 void* sync_ws, const float* old_mean = nullptr, const float* old_std = nullptr, float kl_bound = 0.f, float pg_coef = 0.f) {
  fill_run(a, theta, adam_m, adam_v, adam_step_critics, obs, act, logp_old, target_r, target_c, adv, perm, M, cfg, n_nets, first_net,
           stale_io, losses, sync_ws);
  a.pow_b1_actor = pow((double)cfg.beta1, (double)adam_step_actor);
  a.pow_b2_actor = pow((double)cfg.beta2, (double)adam_step_actor);
  a.old_mean = old_mean; a.old_std = old_std; a.kl_bound = kl_bound; a.pg_coef = pg_coef;
}

}  // namespace spo
