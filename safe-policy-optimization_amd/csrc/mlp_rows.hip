// One-launch minibatch gradient of the wide-network path, split over the ROWS (round 6).  gfx950 only.
//
// The wide path (any hidden_sizes: reference safepo/common/model.py:30-48,131; the minibatch step safepo/single_agent/ppo_lag.py:306-324)
// took a step of the reference's default 64-row minibatch as gather + one-workgroup-per-network forward (csrc/mlp_small.hip) + loss +
// one-workgroup-per-network backward + three optimiser launches: 89 us at hidden [128, 128], of which 24 + 36 us are the two
// mlp_small launches -- one CU per network staging every weight matrix through LDS behind barriers.  Nothing in forward / loss /
// backward couples the ROWS of a minibatch except the sums over rows in the weight gradients and the loss values, so here a
// workgroup carries ONE 16-row group of ONE network through all of it:
//   * grid = networks x ceil(rows / 16) workgroups of 8 waves; no workgroup waits for another (no exchange, no co-residency need);
//   * the rows are read through the minibatch's index window (perm[cursor .. cursor + rows): the DataLoader batch of
//     ppo_lag.py:298-305) -- no gather launch;
//   * activations of every level live in LDS twice: a row image [16][width + 4] (B operand of the next layer, 1 - h^2 of the
//     backward) and a transposed image [width][16 + 4] (B operand of the weight-gradient product, whose reduction index is the
//     row); dZ likewise (row image: B operand of dH = dZ W; transposed: A operand of dW = dZ^T H);
//   * weights come straight from global memory as MFMA A fragments (16 bytes per lane): 8 waves deal the 16-unit output tiles, so
//     no weight is staged and no barrier sits inside a layer -- one barrier per layer each way; a wave's first tile of the NEXT
//     layer (eight input tiles: all of a 128-wide layer) is requested a whole stage ahead into a second register set;
//   * the loss of the network (MSE of a critic, the clipped surrogate and d(log_std) of the actor: the arithmetic of
//     wide_ppo_loss_kernel, csrc/wide.hip) is evaluated between forward and backward on the 16 rows, with the GLOBAL 1 / rows;
//   * every workgroup writes its row group's PARTIAL gradient (theta's layout) and loss sums to parts[group]; a second, tiny launch
//     (spo_wide_reduce_parts) adds the groups in fixed order into the flat gradient -- deterministic, and exactly where the
//     data-parallel all-reduce and spo_wide_clip_adam take over.
//   * the KL-penalty loss of FOCOPS / CUP's second stage (focops.py:326-347, cup.py:370-386) is a second loss form of the same kernel
//     (the LOSS template parameter): its gradient is g_KL + F g_PG with F the minibatch's fraction of rows inside the KL bound, both
//     parts sums over rows, so the actor runs in two kinds of workgroup -- one cotangent each, see mlp_rows_grad_kernel -- and the
//     group sum (spo_wide_kl_penalty_reduce_parts) combines them, or leaves them apart for a data-parallel all-reduce.  Measured
//     (profiles/klpen_rows/): the launch 1.06 x the PPO launch's time, the FOCOPS step at [128, 128] 84 -> 36 us.
//   * several independent runs of one shape share the step's launches (the seed-batched forms, `--seeds`): run r is the grid slice
//     blockIdx.y == r, reads what its stand-alone launch receives as kernel arguments from its entry of a device table (uniform
//     index: scalar loads) and runs the same body on the stand-alone blockIdx.x / gridDim.x -- bit for bit its own step; a run with
//     active == 0 returns at once.  No workgroup waits for another, so nothing caps the runs but the table (32).  The fused
//     PPO-Lagrangian step in three launches: spo_wide_rows_step_multi.  The FOCOPS / CUP step (KL penalty with or without the
//     critics, and CUP's first stage with the clipped surrogate) in its five -- the gradient launch and the group sum here, the
//     three optimiser launches of csrc/wide.hip through csrc/wide_opt.h: spo_wide_rows_ex_step_multi; its table is
//     [S x MrMultiEntry | S x MrRedEntry | S x the optimiser's entry].
// fp32 v_mfma_f32_16x16x4_f32 throughout (bitwise an fmaf chain); results differ from the launch-per-layer path in summation
// order only.
// Measured (hidden [128, 128], 60 / 8, 64 rows, one MI355X, profiles/r06/wide_step.txt, wide_rows_phase_cycles.txt): the kernel
// 19-19.6 us (of a 30.1 us step) of which ~4 us are MFMA issue time (1 120 useful v_mfma per workgroup, two waves per SIMD), the rest the serial chain of
// a stage -- B-operand reads, the MFMA chain, tanh, image stores, barrier -- nine times, plus cursor -> index -> observation rows
// (three dependent round trips, 2.7 us).  What did NOT help, each measured: warming the XCD's L2 with the parameters at the
// kernel's start (32.3 against 32.6 us per step), eight-tile load batches without the prefetch (slower: the loads are not the
// bound), requesting the next layer behind the current layer's MFMAs instead of in front of them (no change).  What did: the
// host-tabulated LDS map (-1.7 us: mr_level's loops were dependent scalar loads at every stage), skipping tile pairs beyond a
// layer's width (-1 us), one kernel body per load form (the VEC template parameter: with both forms in one body the compiler
// fenced every fragment's load behind the other form's registers).
#include "common.h"
#include "mlp_mfma.h"
#include "adam.h"
#include "adam_host.h"
#include <cstdlib>
#include <vector>
#include "wide_opt.h"
#include "../../include/safepo_hip.h"

namespace {
using namespace spo;

constexpr int MR_TS = 20;                          // row stride of a transposed image: 16 rows + 4 (16-byte aligned, bank-rotated)
constexpr int MR_MAX_GROUPS = 16;                  // row groups of one launch (256 rows)
constexpr size_t MR_MAX_LDS = 160 * 1024;          // all of a CU's LDS (the kernel has no static LDS): [256, 256] at 60 / 8 needs 157.4 KB
// behind the images: row indices (int64[16]), per-row scalars, log_std and 1 / sigma^2, the d(log_std) terms, the rows' actions
// (the act_dim-sized pieces at the launch's act_dim rounded up to 4 -- AP -- so that a narrow action vector leaves the space to the images)
constexpr int MR_RIDX = 0, MR_ROWA = 32, MR_ROWL = 48, MR_RADV = 64, MR_RLOGP = 80, MR_RTGT = 96, MR_LS = 112;
__host__ __device__ inline int mr_ap(int A) { return A < 1 ? 4 : (A + 3) & ~3; }
__host__ __device__ inline int mr_ivar(int AP) { return MR_LS + AP; }
__host__ __device__ inline int mr_dls(int AP) { return MR_LS + 2 * AP; }
__host__ __device__ inline int mr_ract(int AP) { return MR_LS + 2 * AP + 16 * AP; }
__host__ __device__ inline int mr_misc(int AP) { return MR_LS + 2 * AP + 32 * AP; }
// the KL-penalty launch only (behind mr_misc): the rows' old means [16][act_dim], then 1 / old_std, the variance ratio and its log
__host__ __device__ inline int mr_klx(int AP) { return 16 * AP + 3 * AP; }
enum { MR_PPO = 0, MR_KLPEN = 1 };                  // loss form of a launch (template parameter of the gradient kernel)

constexpr float LOG_SQRT_2PI_F = 0.91893853320467274178f;               // (mlp_mfma.h's LOG_SQRT_2PI)
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));      // four consecutive floats at any dword address

struct MrNet {
  int n;                                           // Linear layers
  int kind;                                        // 0 reward critic, 1 cost critic, 2 actor (KL-penalty launch: its KL part), 3 actor again (PG part)
  int d[SPO_MLP_MAX_LAYERS + 1];                   // widths: d[0] = obs_dim, d[n] = 1 or act_dim
  int64_t w[SPO_MLP_MAX_LAYERS], b[SPO_MLP_MAX_LAYERS];   // offsets of W_l [d[l+1]][d[l]] and b_l in theta
  // the LDS map (mr_level / mr_pz / mr_images_end), tabulated by the host: the kernel reads an entry with one scalar load where the
  // loops of mr_level cost it a chain of dependent ones at every stage (~1 us per stage, measured)
  int pr[SPO_MLP_MAX_LAYERS + 1], hr[SPO_MLP_MAX_LAYERS + 1], ht[SPO_MLP_MAX_LAYERS + 1];
  int pz, zbase;
  int64_t poff;                                    // KL-penalty launch: where this network's partial gradient sits in a group's part, minus w[0]'s block
};
struct MrArgs {
  const float* theta; const float* obs; const float* act; const float* logp_old; const float* tgt_r; const float* tgt_c; const float* adv;
  const int64_t* idx; const int64_t* cursor;
  float* parts; int64_t stride; int64_t P; int64_t ls_off;
  int rows, R, n_nets, A;
  float clip;
  const float* old_mean; const float* old_std;     // KL-penalty launch: old_mean[M][act_dim] (read through the index window), old_std[act_dim]
  float kl_bound, pg_coef;
  MrNet net[4];
};

struct MrOptArgs {
  const float* parts; int R; int64_t stride;
  float* theta; float* grad; float* m; float* v; int64_t P, r_end, c_end, actor_begin; int64_t rows;
  float l2, vcoef_r, max_norm, lr_actor, lr_critic, b1, b2, eps;
  float w1, w2;                      // 1 - beta1, 1 - beta2 formed on the host in double (csrc/adam_host.h), as wide_adam_kernel takes them
  double b1d, b2d;                   // the betas the caller meant: the optimiser clocks are their powers (as wide_coef_kernel's)
  double* partial; float* scal; float* losses3; double* pow4;
  float* loss_log; int64_t* cursor; int64_t cursor_step; int nblocks;
};
// the seed-batched step's device table: per run the arguments of its stand-alone launches; MrKernArg: a kernel's parameter type
struct MrMultiEntry {
  MrArgs g;
  MrOptArgs o;
  int active;
};
template <bool MULTI> struct MrKernArg {
  typedef MrArgs Grad;
  typedef MrOptArgs Opt;
  static __device__ __forceinline__ const MrOptArgs& opt(const MrOptArgs& x) { return x; }
};
template <> struct MrKernArg<true> {
  typedef const MrMultiEntry* __restrict__ Grad;
  typedef const MrMultiEntry* __restrict__ Opt;
  static __device__ __forceinline__ const MrOptArgs& opt(const MrMultiEntry* __restrict__ t) { return t[blockIdx.y].o; }
};

__host__ __device__ inline int mr_up16(int v) { return (v + 15) & ~15; }
__device__ __forceinline__ int imin_(int a, int b) { return a < b ? a : b; }

// LDS map of a network: level v (0 = the observations, v = output of layer v) has a row image at hr and, below the output level, a
// transposed image at ht; behind them two dZ row images and two transposed ones (ping-pong over the layers), then mr_misc() floats.
struct MrLevel { int pr, hr, ht; };
__host__ __device__ inline MrLevel mr_level(const MrNet& nn, int v) {
  MrLevel L{0, 0, 0};
  int off = 0;
  for (int u = 0; u <= v; ++u) {
    L.pr = mr_up16(nn.d[u]);
    L.hr = off; off += 16 * (L.pr + 4);
    L.ht = off;
    if (u < nn.n) off += L.pr * MR_TS;
  }
  return L;
}
__host__ __device__ inline int mr_pz(const MrNet& nn) {
  int pz = 16;
  for (int u = 1; u <= nn.n; ++u) pz = mr_up16(nn.d[u]) > pz ? mr_up16(nn.d[u]) : pz;
  return pz;
}
__host__ __device__ inline int mr_images_end(const MrNet& nn) {
  const MrLevel L = mr_level(nn, nn.n);
  return L.hr + 16 * (L.pr + 4);
}
__host__ __device__ inline int mr_lds_floats(const MrNet& nn, int A) {
  const int pz = mr_pz(nn);
  return mr_images_end(nn) + 2 * 16 * (pz + 4) + 2 * pz * MR_TS + mr_misc(mr_ap(A));
}

// A fragment of a row-major weight row: W[row][16 nt + 4q .. + 3] (vec: K % 4 == 0, one 16-byte load at any dword address;
// otherwise four clamped dword loads).  Columns >= K hold finite garbage: the B operand is zero there.
template <bool VEC>
__device__ __forceinline__ f4 load_w_frag(const float* __restrict__ wr, int K, int nt, int q) {
  const int k0 = 16 * nt + 4 * q;
  f4 v;
  if constexpr (VEC) {
    const f4u t = *reinterpret_cast<const f4u*>(wr + imin_(k0, K - 4));
    v = f4{t[0], t[1], t[2], t[3]};
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = wr[imin_(k0 + r, K - 1)];
  }
  return v;
}

// The A fragments of eight input tiles nt0 .. nt0 + 7 of a weight row (clamped beyond KT: their B operands are zeroed) -- ONE
// memory round trip for a 128-wide layer; the caller issues them a stage ahead where it can.
// (VEC is a property of the LAUNCH -- every layer's input width a multiple of 4 -- not a run-time branch: with both forms in one
// body the compiler's wait-count bookkeeping fenced each load of one form behind the registers of the other, a serial round trip
// per fragment, measured)
template <bool VEC>
__device__ __forceinline__ void load_a8(const float* __restrict__ wr, int K, int KT, int nt0, int q, f4 (&av)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) av[i] = load_w_frag<VEC>(wr, K, imin_(nt0 + i, KT - 1), q);
}
__device__ __forceinline__ void mma8(const f4 (&av)[8], const float* hin, int KT, int nt0, f4& acc0, f4& acc1) {
  f4 bv[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const f4 t = *reinterpret_cast<const f4*>(hin + 16 * imin_(nt0 + i, KT - 1));
    bv[i] = nt0 + i < KT ? t : f4{0.f, 0.f, 0.f, 0.f};
  }
  // (tile pairs beyond the layer's width are skipped -- a wave-uniform branch per eight MFMAs: a 64-wide input is half a batch)
#pragma unroll
  for (int i = 0; i < 8; i += 2) {
    if (i == 0 || nt0 + i < KT) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        acc0 = mfma4(av[i][r], bv[i][r], acc0);
        acc1 = mfma4(av[i + 1][r], bv[i + 1][r], acc1);
      }
    }
  }
}
// the same for dH = dZ W: A[in-unit kcol][u] = W[u][kcol] for the eight unit tiles ut0 .. ut0 + 7 (32 dword loads, one round trip)
__device__ __forceinline__ void load_t8(const float* __restrict__ W, int K, int N, int NT, int ut0, int kcol, int q, float (&av)[8][4]) {
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) av[i][r] = W[(int64_t)imin_(16 * imin_(ut0 + i, NT - 1) + 4 * q + r, N - 1) * K + kcol];
}
__device__ __forceinline__ void mma_t8(const float (&av)[8][4], const float* zb, int NT, int ut0, f4& acc0, f4& acc1) {
  f4 bv[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const f4 t = *reinterpret_cast<const f4*>(zb + 16 * imin_(ut0 + i, NT - 1));
    bv[i] = ut0 + i < NT ? t : f4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int i = 0; i < 8; i += 2) {
    if (i == 0 || ut0 + i < NT) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        acc0 = mfma4(av[i][r], bv[i][r], acc0);
        acc1 = mfma4(av[i + 1][r], bv[i + 1][r], acc1);
      }
    }
  }
}

#ifdef SPO_MR_PROF
// development aid (tools/build_variant.py mrprof -DSPO_MR_PROF, SPO_VARIANT_SOURCES=mlp_rows.hip): wall-clock stamps (100 MHz) of
// the first lane of workgroups 0 and gridDim - 1 at the stage boundaries
__device__ unsigned long long g_mr_prof[2][32];
#define MR_STAMP(k) do { const int k_ = (k); if (threadIdx.x == 0 && (blockIdx.x == 0 || blockIdx.x == gridDim.x - 1) && k_ < 32) \
  g_mr_prof[blockIdx.x == 0 ? 0 : 1][k_] = wall_clock64(); } while (0)
#else
#define MR_STAMP(k) do { } while (0)
#endif

// LOSS == MR_KLPEN (FOCOPS focops.py:326-347, CUP's second stage cup.py:370-386): the actor runs in TWO kinds of workgroup, both
// with its forward on their 16 rows -- kind 2 backpropagates ind_i d(KL_i)/d(mean) / rows, kind 3 -(pg_coef / rows) d(ratio_i adv_i)/d(mean)
// (the fraction F of rows inside the bound taken as 1: the loss's gradient is g_KL + F g_PG, and F is known once every row's
// indicator is, i.e. in the group sum behind this launch).  One cotangent per workgroup: the backward stages are those of the
// clipped surrogate.  Per-row arithmetic: wide_klpen_split_kernel's (csrc/wide.hip).
// MULTI (the seed-batched launch, spo_wide_rows_step_multi): the same body for run blockIdx.y of S independent runs of one shape -- `a` is
// then that run's entry of a device table (what its stand-alone launch receives as kernel arguments; uniform index, const
// __restrict__: scalar loads) instead of the kernel-argument struct.  blockIdx.x and gridDim.x are the stand-alone launch's, no
// block waits for another: run r is a slice of the grid.  A block of a run with active == 0 returns before it touches anything else.
template <bool VEC, int LOSS = MR_PPO, bool MULTI = false>
__global__ __launch_bounds__(512) void mlp_rows_grad_kernel(typename MrKernArg<MULTI>::Grad arg) {
  const MrArgs* ap;
  if constexpr (MULTI) {
    if (!arg[blockIdx.y].active) return;
    ap = &arg[blockIdx.y].g;
  } else ap = &arg;
  const MrArgs& a = *ap;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, j = lane & 15, q = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int net = blockIdx.x / a.R, rg = blockIdx.x - net * a.R;
  const MrNet& nn = a.net[net];
  const int n = nn.n, kind = nn.kind;
  const int row0 = 16 * rg, nrows = imin_(16, a.rows - row0);
  const int PZ = nn.pz, ZS = PZ + 4;
  const int zbase = nn.zbase;
  float* const misc = lds + zbase + 2 * 16 * ZS + 2 * PZ * MR_TS;
  long long* const ridx = reinterpret_cast<long long*>(misc + MR_RIDX);   // [16] (the map's pieces are multiples of 4 floats)
  float* const rowa = misc + MR_ROWA;                                   // [16] d(loss)/d(log-prob) (actor) or d(loss)/d(value)
  float* const rowl = misc + MR_ROWL;                                   // [16] the row's loss term
  const int AP = mr_ap(a.A), MR_IVAR = mr_ivar(AP);
  float* const dls = misc + mr_dls(AP);                                 // [act_dim][16] d(log_std) terms
  float* const ract = misc + mr_ract(AP);                               // [16][act_dim] the rows' actions
  float* const gpart = a.parts + (int64_t)rg * a.stride;                // this group's part (the row sums sit at gpart[P ..])
  float* const part = LOSS == MR_KLPEN ? gpart + nn.poff : gpart;
  float* const klx = misc + mr_misc(AP);                                // KL-penalty launch: [16][act_dim] old means, 1 / old_std, vrat, log vrat
  const bool isact = LOSS == MR_KLPEN ? kind >= 2 : kind == 2;
  const int OUT = nn.d[n];
  int stamp = 0;
  MR_STAMP(stamp++);

  // ---- the minibatch's rows of this group (clamped: rows beyond the minibatch repeat its last row and carry a zero dZ)
  if (tid < 16) {
    const int64_t base = a.cursor ? a.cursor[0] : 0;
    const int64_t at = base + row0 + imin_(tid, nrows - 1);
    ridx[tid] = a.idx ? a.idx[at] : at;
  }
  if (isact && tid >= 64 && tid < 64 + OUT) {
    const float ls = a.theta[a.ls_off + tid - 64], sd = __expf(ls);
    misc[MR_LS + tid - 64] = ls;
    misc[MR_IVAR + tid - 64] = 1.f / (sd * sd);
    if constexpr (LOSS == MR_KLPEN) {
      const float iso = 1.f / a.old_std[tid - 64];
      const float sr = sd * iso;                     // kl_normal_normal: var_ratio = (p.scale / q.scale)^2
      const float vrat = sr * sr;
      klx[16 * AP + tid - 64] = iso; klx[17 * AP + tid - 64] = vrat; klx[18 * AP + tid - 64] = logf(vrat);
    }
  }
  // the weights of a wave's FIRST output tile of a layer (its first eight input tiles) and that tile's biases, requested one stage
  // ahead of their use -- before the barrier that publishes their B operand
  f4 pre[8], pbias, nxt[8], nbias;
  auto prefetch_fwd = [&](int l, f4 (&dst)[8], f4& dbias) {
    const int K = nn.d[l], N = nn.d[l + 1], KT = nn.pr[l] >> 4;
    const float* __restrict__ W = a.theta + nn.w[l];
    const float* __restrict__ bias = a.theta + nn.b[l];
    const int mt = imin_(wave, (nn.pr[l + 1] >> 4) - 1);
    // (biases first: behind the weights the compiler put a full vmcnt(0) in front of them -- a round trip on the critical path)
#pragma unroll
    for (int r = 0; r < 4; ++r) dbias[r] = bias[imin_(16 * mt + 4 * q + r, N - 1)];
    load_a8<VEC>(W + (int64_t)imin_(16 * mt + j, N - 1) * K, K, KT, 0, q, dst);
  };
  prefetch_fwd(0, pre, pbias);
  __syncthreads();
  MR_STAMP(stamp++);
  {
    // observations -> both images of level 0; the loss's per-row inputs -> LDS now, so that the loss stage waits for no global load
    const MrLevel L0{nn.pr[0], nn.hr[0], nn.ht[0]};
    const int D = nn.d[0], S0 = L0.pr + 4;
    for (int r = wave; r < 16; r += 8) {
      const float* __restrict__ src = a.obs + ridx[r] * (int64_t)D;
      for (int c = lane; c < L0.pr; c += 64) {
        const float v = (r < nrows && c < D) ? src[imin_(c, D - 1)] : 0.f;
        lds[L0.hr + r * S0 + c] = v;
        lds[L0.ht + c * MR_TS + r] = v;
      }
      if (isact) {
        const float* __restrict__ sa = a.act + ridx[r] * (int64_t)OUT;
        for (int c = lane; c < OUT; c += 64) ract[r * OUT + c] = sa[c];
        if constexpr (LOSS == MR_KLPEN) {
          const float* __restrict__ so = a.old_mean + ridx[r] * (int64_t)OUT;
          for (int c = lane; c < OUT; c += 64) klx[r * OUT + c] = so[c];
        }
      }
    }
    if (tid >= 448 && tid < 464) {
      const int64_t gi = ridx[tid - 448];
      misc[MR_RTGT + tid - 448] = kind == 0 ? a.tgt_r[gi] : (kind == 1 ? a.tgt_c[gi] : 0.f);
      if (isact) { misc[MR_RADV + tid - 448] = a.adv[gi]; misc[MR_RLOGP + tid - 448] = a.logp_old[gi]; }
    }
  }
  __syncthreads();
  MR_STAMP(stamp++);

  // ---- forward: h_{l+1} = tanh(W_l h_l + b_l); wave w takes the output tiles w, w + 8, ...
  for (int l = 0; l < n; ++l) {
    const MrLevel Li{nn.pr[l], nn.hr[l], nn.ht[l]}, Lo{nn.pr[l + 1], nn.hr[l + 1], nn.ht[l + 1]};
    const int K = nn.d[l], N = nn.d[l + 1], KT = Li.pr >> 4, NT = Lo.pr >> 4, SO = Lo.pr + 4;
    const float* __restrict__ W = a.theta + nn.w[l];
    const float* __restrict__ bias = a.theta + nn.b[l];
    const bool act = l + 1 < n;
    const float* hin = lds + Li.hr + j * (Li.pr + 4) + 4 * q;
    // the NEXT layer's first tile: requested a whole stage ahead, into a second register set (the one in use is busy; a request
    // behind this layer's MFMAs left the loads ~0.5 us before their use and the next layer waited out the rest of the round trip)
    if (l + 1 < n) prefetch_fwd(l + 1, nxt, nbias);
    for (int mt = wave; mt < NT; mt += 8) {
      const int u0 = 16 * mt + 4 * q;
      const float* __restrict__ wr = W + (int64_t)imin_(16 * mt + j, N - 1) * K;
      f4 acc0, acc1 = f4{0.f, 0.f, 0.f, 0.f};
      if (mt == wave) {
        acc0 = pbias;
        mma8(pre, hin, KT, 0, acc0, acc1);
      } else {
        f4 av[8];
        load_a8<VEC>(wr, K, KT, 0, q, av);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc0[r] = bias[imin_(u0 + r, N - 1)];
        mma8(av, hin, KT, 0, acc0, acc1);
      }
      for (int nt0 = 8; nt0 < KT; nt0 += 8) {
        f4 av[8];
        load_a8<VEC>(wr, K, KT, nt0, q, av);
        mma8(av, hin, KT, nt0, acc0, acc1);
      }
      MR_STAMP(16 + 4 * l);
      f4 v = acc0 + acc1;
      if (act) v = fast_tanh4(v);
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = u0 + r < N ? v[r] : 0.f;
      *reinterpret_cast<f4*>(lds + Lo.hr + j * SO + u0) = v;
      if (act) {
#pragma unroll
        for (int r = 0; r < 4; ++r) lds[Lo.ht + (u0 + r) * MR_TS + j] = v[r];
      }
    }
    MR_STAMP(17 + 4 * l);
    if (l + 1 < n) {
#pragma unroll
      for (int i = 0; i < 8; ++i) pre[i] = nxt[i];
      pbias = nbias;
    }
    MR_STAMP(18 + 4 * l);
    __syncthreads();
    MR_STAMP(stamp++);
  }

  // dH = dZ W of layer l: the weights of this wave's first input-unit tile (first eight unit tiles), a stage ahead
  float pt[8][4], npt[8][4];
  auto prefetch_bwd = [&](int l, float (&dst)[8][4]) {
    const int K = nn.d[l], N = nn.d[l + 1], NT = nn.pr[l + 1] >> 4;
    const int mt = imin_(wave, (nn.pr[l] >> 4) - 1);
    load_t8(a.theta + nn.w[l], K, N, NT, 0, imin_(16 * mt + j, K - 1), q, dst);
  };
  if (n > 1) prefetch_bwd(n - 1, pt);
  // ---- loss of this network on the group's rows -> d(loss)/d(output) in the first dZ images (zero beyond the rows / the outputs)
  float* ZR = lds + zbase;
  float* ZT = lds + zbase + 2 * 16 * ZS;
  const MrLevel Ln{nn.pr[n], nn.hr[n], nn.ht[n]};
  const int SN = Ln.pr + 4;
  const float inv_n = 1.f / (float)a.rows;
  if (tid < 16) {
    const int r = tid;
    float da = 0.f, lt = 0.f;
    [[maybe_unused]] float cnt = 0.f;
    if (r < nrows) {
      if (kind < 2) {                                    // MSE of a critic (ppo_lag.py:306-309)
        const float diff = lds[Ln.hr + r * SN] - misc[MR_RTGT + r];
        lt = diff * diff;
        da = 2.f * diff * inv_n;
      } else if (LOSS == MR_KLPEN && kind == 2) {        // ind_i KL_i and its indicator (focops.py:326-333)
        float kl = 0.f;
        for (int k = 0; k < OUT; ++k) {
          const float dm = (lds[Ln.hr + r * SN + k] - klx[r * OUT + k]) * klx[16 * AP + k];       // (loc_p - loc_q) / scale_q
          kl += 0.5f * (klx[17 * AP + k] + dm * dm - 1.f - klx[18 * AP + k]);
        }
        const float ind = (kl <= a.kl_bound) ? 1.f : 0.f;
        da = ind * inv_n;
        lt = ind * kl;
        cnt = ind;
      } else if (LOSS == MR_KLPEN) {                     // ratio_i adv_i with F taken as 1 (focops.py:334-341)
        float lp = 0.f;
        for (int k = 0; k < OUT; ++k) {
          const float ls = misc[MR_LS + k], ivar = misc[MR_IVAR + k];
          const float dif = ract[r * OUT + k] - lds[Ln.hr + r * SN + k];
          lp += -(dif * dif) * (0.5f * ivar) - ls - LOG_SQRT_2PI_F;
        }
        const float ad = misc[MR_RADV + r];
        const float ratio = __expf(lp - misc[MR_RLOGP + r]);
        da = -(a.pg_coef * ad * ratio) * inv_n;
        lt = ratio * ad;
      } else {                                           // clipped surrogate (ppo_lag.py:316-319): wide_ppo_loss_kernel's arithmetic
        const float clip_lo = 1.f - a.clip, clip_hi = 1.f + a.clip;
        float lp = 0.f;
        for (int k = 0; k < OUT; ++k) {
          const float ls = misc[MR_LS + k], ivar = misc[MR_IVAR + k];
          const float dif = ract[r * OUT + k] - lds[Ln.hr + r * SN + k];
          lp += -(dif * dif) * (0.5f * ivar) - ls - LOG_SQRT_2PI_F;
        }
        const float ad = misc[MR_RADV + r];
        const float ratio = __expf(lp - misc[MR_RLOGP + r]);
        const float rc = fminf(fmaxf(ratio, clip_lo), clip_hi);
        const float s1 = ratio * ad, s2 = rc * ad;
        const bool inr = (ratio >= clip_lo) && (ratio <= clip_hi);
        float gr;                                        // backward of torch.min / torch.clamp (ties split the gradient)
        if (s1 < s2) gr = ad;
        else if (s1 > s2) gr = inr ? ad : 0.f;
        else gr = 0.5f * ad + (inr ? 0.5f * ad : 0.f);
        da = -(gr * ratio) * inv_n;
        lt = fminf(s1, s2);
      }
    }
    rowa[r] = da; rowl[r] = lt;
    if constexpr (LOSS == MR_KLPEN) misc[MR_RTGT + r] = cnt;     // (the targets' slot: an actor's workgroup has none)
  }
  __syncthreads();
  for (int e = tid; e < 16 * Ln.pr; e += 512) {
    const int r = e & 15, u = e >> 4;
    float dz = 0.f;
    if (u < OUT && r < nrows) {
      if (kind < 2) dz = rowa[r];
      else if (LOSS == MR_KLPEN && kind == 2) {
        const float iso = klx[16 * AP + u];
        const float dm = (lds[Ln.hr + r * SN + u] - klx[r * OUT + u]) * iso;
        dz = rowa[r] * dm * iso;
        dls[u * 16 + r] = rowa[r] * (klx[17 * AP + u] - 1.f);
      } else {
        const float ivar = misc[MR_IVAR + u];
        const float dif = ract[r * OUT + u] - lds[Ln.hr + r * SN + u];
        const float z = dif * ivar;
        dz = rowa[r] * z;
        dls[u * 16 + r] = rowa[r] * (dif * z - 1.f);
      }
    } else if (isact && u < OUT) dls[u * 16 + r] = 0.f;
    ZR[r * ZS + u] = dz;
    ZT[u * MR_TS + r] = dz;
  }
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int r = 0; r < 16; ++r) s += (double)rowl[r];
    if constexpr (LOSS == MR_KLPEN) {
      // a group's row sums: [P + 0 / 1] the critics' squared errors, [P + 2] count of ind, [P + 3] sum ind*KL, [P + 4] sum ratio*adv
      if (kind == 2) {
        double c = 0.0;
        for (int r = 0; r < 16; ++r) c += (double)misc[MR_RTGT + r];
        gpart[a.P + 2] = (float)c; gpart[a.P + 3] = (float)s;
      } else gpart[a.P + (kind == 3 ? 4 : kind)] = (float)s;
    } else part[a.P + kind] = (float)s;
  }
  if (isact && tid >= 64 && tid < 64 + OUT) {
    const int u = tid - 64;
    double s = 0.0;
    for (int r = 0; r < 16; ++r) s += (double)dls[u * 16 + r];
    part[a.ls_off + u] = (float)s;
  }

  MR_STAMP(stamp++);
  // ---- backward: db, dW (this group's rows) and dZ of the layer below; one barrier per layer
  int cur = 0;
  for (int l = n - 1; l >= 0; --l) {
    const MrLevel Li{nn.pr[l], nn.hr[l], nn.ht[l]}, Lo{nn.pr[l + 1], nn.hr[l + 1], nn.ht[l + 1]};
    const int K = nn.d[l], N = nn.d[l + 1], KT = Li.pr >> 4, NT = Lo.pr >> 4, SI = Li.pr + 4;
    const float* __restrict__ W = a.theta + nn.w[l];
    const float* ZRc = ZR + cur * 16 * ZS;
    const float* ZTc = ZT + cur * PZ * MR_TS;
    float* ZRn = ZR + (cur ^ 1) * 16 * ZS;
    float* ZTn = ZT + (cur ^ 1) * PZ * MR_TS;
    float* __restrict__ pW = part + nn.w[l];
    float* __restrict__ pb = part + nn.b[l];
    if (l > 1) prefetch_bwd(l - 1, npt);                 // (a whole stage ahead, second register set: see the forward)
    // (1) bias gradient: the column sums of dZ in row order
    for (int u = tid; u < N; u += 512) {
      float s = 0.f;
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const f4 t = *reinterpret_cast<const f4*>(ZTc + u * MR_TS + 4 * r4);
        s += t[0]; s += t[1]; s += t[2]; s += t[3];
      }
      pb[u] = s;
    }
    if (l == 1) MR_STAMP(26);
    // (2) weight gradient dW[u][k] = sum_rows dZ[row][u] h[row][k]: tiles (unit tile, input tile) dealt to the waves; the reduction
    //     index is the row -- four MFMAs per tile
    {
      const float* za = ZTc + j * MR_TS + 4 * q;
      const float* hb = lds + Li.ht + j * MR_TS + 4 * q;
      const int ntile = NT * KT;
      // (the tile's coordinates advance without a division -- p / KT with a run-time KT is ~40 scalar instructions per tile -- and
      //  the store offsets are 32-bit on the uniform base.  Four tiles per round with their sixteen MFMAs interleaved, and the
      //  stores left out altogether, measured the same 0.3 us per tile: neither the dependent MFMAs nor the stores are the bound.)
      int mt = wave / KT, nt = wave - mt * KT;
#pragma unroll 2
      for (int p = wave; p < ntile; p += 8, nt += 8) {
        while (nt >= KT) { nt -= KT; ++mt; }
        const f4 av = *reinterpret_cast<const f4*>(za + 16 * mt * MR_TS);
        const f4 bv = *reinterpret_cast<const f4*>(hb + 16 * nt * MR_TS);
        f4 acc = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 4; ++r) acc = mfma4(av[r], bv[r], acc);
        const int col = 16 * nt + j, u0 = 16 * mt + 4 * q;
        if (col < K) {
          const unsigned off = (unsigned)(u0 * K + col);
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (u0 + r < N) pW[off + (unsigned)(r * K)] = acc[r];
        }
      }
    }
    if (l == 1) MR_STAMP(27);
    // (3) dZ of the layer below: dH = dZ W, dZ' = dH (1 - h^2); wave w takes the input-unit tiles w, w + 8, ...; the first
    //     tile's weights were requested a stage ahead (pt)
    if (l > 0) {
      const float* zb = ZRc + j * ZS + 4 * q;
      for (int mt = wave; mt < KT; mt += 8) {
        const int kcol = imin_(16 * mt + j, K - 1);
        f4 acc0 = f4{0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
        if (mt == wave) mma_t8(pt, zb, NT, 0, acc0, acc1);
        else {
          float av[8][4];
          load_t8(W, K, N, NT, 0, kcol, q, av);
          mma_t8(av, zb, NT, 0, acc0, acc1);
        }
        for (int ut0 = 8; ut0 < NT; ut0 += 8) {
          float av[8][4];
          load_t8(W, K, N, NT, ut0, kcol, q, av);
          mma_t8(av, zb, NT, ut0, acc0, acc1);
        }
        const f4 dh = acc0 + acc1;
        const int u0 = 16 * mt + 4 * q;
        const f4 h = *reinterpret_cast<const f4*>(lds + Li.hr + j * SI + u0);
        f4 dz;
#pragma unroll
        for (int r = 0; r < 4; ++r) dz[r] = u0 + r < K ? dh[r] * fmaf(-h[r], h[r], 1.f) : 0.f;
        *reinterpret_cast<f4*>(ZRn + j * ZS + u0) = dz;
#pragma unroll
        for (int r = 0; r < 4; ++r) ZTn[(u0 + r) * MR_TS + j] = dz[r];
      }
    }
    if (l == 1) MR_STAMP(28);
    if (l > 1) {
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) pt[i][r] = npt[i][r];
    }
    if (l == 1) MR_STAMP(29);
    __syncthreads();
    MR_STAMP(stamp++);
    cur ^= 1;
  }
}

// grad[i] = sum over the row groups of parts[g][i] (group order), losses3 = the three data losses of the minibatch
// (the body as text, on the names parts / R / stride / P / rows / n_loss / grad / losses: the stand-alone kernel has them as its
//  eight scalar parameters, the table-driven one below as locals read from its run's entry.  A shared device function, inlined,
//  reordered two operands of the stand-alone kernel's instructions; this way its code is what it was.)
#define MR_REDUCE_BODY                                                                                                  \
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < P; i += (int64_t)gridDim.x * 256) {                     \
    float s = parts[i];                                                                                                 \
    for (int g = 1; g < R; ++g) s += parts[(int64_t)g * stride + i];                                                    \
    grad[i] = s;                                                                                                        \
  }                                                                                                                     \
  if (blockIdx.x == 0 && threadIdx.x < n_loss && losses) {                                                              \
    double s = 0.0;                                                                                                     \
    for (int g = 0; g < R; ++g) s += (double)parts[(int64_t)g * stride + P + threadIdx.x];                              \
    losses[threadIdx.x] = (float)((threadIdx.x == 2 ? -s : s) / (double)rows);                                          \
  }
__global__ __launch_bounds__(256) void mlp_rows_reduce_kernel(const float* __restrict__ parts, int R, int64_t stride, int64_t P, int64_t rows,
                                                              int n_loss, float* __restrict__ grad, float* __restrict__ losses) {
  MR_REDUCE_BODY
}

// The group sum behind the KL-penalty launch (spo_wide_kl_penalty_reduce_parts).  A group's part: [0, P) the critics' gradients and
// the actor's g_KL, [P, P + 5) its row sums, [pgoff, pgoff + P - ab) the actor's g_PG (F taken as 1).  Groups are added in group
// order; every thread forms the minibatch's row sums itself (<= 16 groups, the same order: the same F in every thread), so the
// combine g_KL + F g_PG needs no second pass.  combine's expressions are wide_klpen_combine_kernel's (csrc/wide.hip) at scale 1.
struct MrKlReduceArgs {
  const float* parts; int R; int64_t stride, P, ab, lo, pgoff, rows;
  int n_loss, combine; float pg_coef;
  float* grad; float* pg_grad; float* sums; float* losses;
};
// MULTI (spo_wide_rows_ex_step_multi): run blockIdx.y's arguments from its entry of a device table (MrRedEntry, below)
struct MrRedEntry;
template <bool MULTI> struct MrRedArg {
  typedef MrKlReduceArgs Kl;
  static __device__ __forceinline__ const MrKlReduceArgs& kl(const MrKlReduceArgs& x) { return x; }
};
template <> struct MrRedArg<true> {
  typedef const MrRedEntry* __restrict__ Kl;
  static __device__ __forceinline__ const MrKlReduceArgs& kl(const MrRedEntry* __restrict__ t);
  static __device__ __forceinline__ bool active(const MrRedEntry* __restrict__ t);
};
template <bool MULTI = false>
__global__ __launch_bounds__(256) void mlp_rows_klpen_reduce_kernel(typename MrRedArg<MULTI>::Kl arg) {
  if constexpr (MULTI) {
    if (!MrRedArg<true>::active(arg)) return;
  }
  const MrKlReduceArgs a = MrRedArg<MULTI>::kl(arg);     // (a copy: the stand-alone kernel's code is then what it was with `a` its parameter)
  double c = 0.0, k = 0.0, ra = 0.0;
  for (int g = 0; g < a.R; ++g) {
    const float* __restrict__ sp = a.parts + (int64_t)g * a.stride + a.P;
    c += (double)sp[2]; k += (double)sp[3]; ra += (double)sp[4];
  }
  const float cnt = (float)c, skl = (float)k, sra = (float)ra, nrow = (float)a.rows;
  const float frac = cnt / nrow;
  for (int64_t i = a.lo + (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.P; i += (int64_t)gridDim.x * 256) {
    float s = a.parts[i];
    for (int g = 1; g < a.R; ++g) s += a.parts[(int64_t)g * a.stride + i];
    if (i >= a.ab) {
      const float* __restrict__ pp = a.parts + a.pgoff + (i - a.ab);
      float p = pp[0];
      for (int g = 1; g < a.R; ++g) p += pp[(int64_t)g * a.stride];
      a.pg_grad[i] = p;
      if (a.combine) s = s + frac * p;
    }
    a.grad[i] = s;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.sums[0] = 0.f; a.sums[1] = 0.f; a.sums[2] = cnt; a.sums[3] = skl; a.sums[4] = sra; a.sums[5] = nrow; a.sums[6] = 0.f; a.sums[7] = 0.f;
    if (a.combine && a.losses) a.losses[2] = (skl - a.pg_coef * frac * sra) / nrow;
  }
  if (blockIdx.x == 0 && threadIdx.x >= 64 && threadIdx.x < 64 + a.n_loss && a.losses) {
    const int q = threadIdx.x - 64;
    double s = 0.0;
    for (int g = 0; g < a.R; ++g) s += (double)a.parts[(int64_t)g * a.stride + a.P + q];
    a.losses[q] = (float)(s / (double)a.rows);
  }
}

// The group sums of the seed-batched FOCOPS / CUP step (spo_wide_rows_ex_step_multi): run blockIdx.y's arguments of
// spo_wide_kl_penalty_reduce_parts (kr) or of spo_wide_reduce_parts (r: CUP's first stage) from its entry of a device table, the
// stand-alone body on the stand-alone blockIdx.x / gridDim.x.  (An entry type of its own: MrMultiEntry keeps its layout, and with it
// the load offsets of the kernels that read it.)
struct MrReduceArgs {
  const float* parts; int R; int64_t stride, P, rows; int n_loss; float* grad; float* losses;
};
struct MrRedEntry {
  MrKlReduceArgs kr;
  MrReduceArgs r;
  int active;
};
__device__ __forceinline__ const MrKlReduceArgs& MrRedArg<true>::kl(const MrRedEntry* __restrict__ t) { return t[blockIdx.y].kr; }
__device__ __forceinline__ bool MrRedArg<true>::active(const MrRedEntry* __restrict__ t) { return t[blockIdx.y].active != 0; }
__global__ __launch_bounds__(256) void mlp_rows_reduce_multi_kernel(const MrRedEntry* __restrict__ tab) {
  if (!tab[blockIdx.y].active) return;
  const MrReduceArgs a = tab[blockIdx.y].r;
  const float* __restrict__ parts = a.parts;
  float* __restrict__ grad = a.grad;
  float* __restrict__ losses = a.losses;
  const int R = a.R, n_loss = a.n_loss;
  const int64_t stride = a.stride, P = a.P, rows = a.rows;
  MR_REDUCE_BODY
}
#undef MR_REDUCE_BODY

// ---- the optimiser behind the row groups in TWO launches (world size 1, device-resident clocks: the replayed step).
// The launch-per-network step ended in wide_prep_kernel -> wide_coef_kernel -> wide_adam_kernel<true> (csrc/wide.hip): with the
// group sum in front, four launches of ~4.5 us that each do < 1 us of work.  Here (1) the group sum, the critics' L2 gradient, the
// value coefficient and the norm partials are one pass over the parameters, whose first workgroup also advances the optimiser
// clocks and the cursor (nobody in that launch reads them), and (2) every workgroup of the Adam pass forms the clip coefficient
// itself from the partials (fixed order: the same value in every workgroup) and reads the advanced clocks; its first workgroup adds
// the L2 terms to the logged losses and stores the loss row.  (A first form kept everything wide_coef_kernel's single lane did in
// the Adam pass behind a device counter -- the last workgroup to arrive wrote the clocks: one same-address atomic per workgroup,
// +20 us a step with 290 workgroups, still +1.5 us with 19 large ones.)  Same arithmetic, element for element, as
// spo_wide_reduce_parts + spo_wide_clip_adam_dev_log.
template <bool MULTI = false>
__global__ __launch_bounds__(256) void mlp_rows_prep_kernel(typename MrKernArg<MULTI>::Opt arg) {
  if constexpr (MULTI) {
    if (!arg[blockIdx.y].active) return;
  }
  const MrOptArgs a = MrKernArg<MULTI>::opt(arg);        // (a copy: the stand-alone kernel's code is then what it was with `a` its parameter)
  __shared__ double red[4][3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double gs = 0.0, pr = 0.0, pc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < a.P; i += (int64_t)gridDim.x * 256) {
    float g = a.parts[i];
    for (int k = 1; k < a.R; ++k) g += a.parts[(int64_t)k * a.stride + i];
    if (i < a.c_end) {
      const float p = a.theta[i];
      g = fmaf(2.f * a.l2, p, g);
      if (i < a.r_end) { g *= a.vcoef_r; pr += (double)(p * p); } else pc += (double)(p * p);
    }
    a.grad[i] = g;
    gs += (double)(g * g);
  }
  gs = wave_sum_d(gs); pr = wave_sum_d(pr); pc = wave_sum_d(pc);
  if (lane == 0) { red[wave][0] = gs; red[wave][1] = pr; red[wave][2] = pc; }
  __syncthreads();
  if (tid < 3) a.partial[(int64_t)blockIdx.x * 3 + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
  if (blockIdx.x == 0 && tid >= 64 && tid < 67) {
    const int k = tid - 64;
    double s = 0.0;
    for (int g = 0; g < a.R; ++g) s += (double)a.parts[(int64_t)g * a.stride + a.P + k];
    a.losses3[k] = (float)((k == 2 ? -s : s) / (double)a.rows);
  }
  // the optimiser clocks and the cursor advance HERE (one lane): nobody in this launch reads them, the gradient launch that did is
  // over, and the Adam pass behind this one reads the advanced clocks as wide_adam_dev_kernel does -- no counter, no atomics
  if (blockIdx.x == 0 && tid == 128) {
    a.pow4[0] *= a.b1d; a.pow4[1] *= a.b2d; a.pow4[2] *= a.b1d; a.pow4[3] *= a.b2d;
    if (a.cursor) a.cursor[0] += a.cursor_step;
  }
}
template <bool MULTI = false>
__global__ __launch_bounds__(256) void mlp_rows_adam_kernel(typename MrKernArg<MULTI>::Opt arg) {
  if constexpr (MULTI) {
    if (!arg[blockIdx.y].active) return;
  }
  const MrOptArgs a = MrKernArg<MULTI>::opt(arg);        // (a copy: the stand-alone kernel's code is then what it was with `a` its parameter)
  __shared__ float sh[4];
  const int tid = threadIdx.x;
  if (tid < 64) {
    // wide_coef_kernel's sum: lane l adds the partials l, l + 64, ... in order, then a fixed butterfly over the lanes
    double gs = 0.0, pr = 0.0, pc = 0.0;
    for (int b = tid; b < a.nblocks; b += 64) { gs += a.partial[b * 3]; pr += a.partial[b * 3 + 1]; pc += a.partial[b * 3 + 2]; }
    gs = wave_sum_d(gs); pr = wave_sum_d(pr); pc = wave_sum_d(pc);
    if (tid == 0) {
      const float norm = sqrtf((float)gs);
      const float coef = a.max_norm / (norm + 1e-6f);              // clip_grad_norm_ (torch): eps 1e-6
      sh[0] = coef > 1.f ? 1.f : coef;
      sh[1] = a.l2 * (float)pr; sh[2] = a.l2 * (float)pc; sh[3] = norm;
    }
  }
  __syncthreads();
  const float coef = sh[0];
  const float lr_a = a.pow4[4] >= 0.0 ? (float)a.pow4[4] : a.lr_actor, lr_c = a.pow4[5] >= 0.0 ? (float)a.pow4[5] : a.lr_critic;
  float ss_a, ss_c, bc2s_a, bc2s_c;
  adam_scalars(lr_a, a.pow4[2], a.pow4[3], ss_a, bc2s_a);            // (advanced by the pass in front: beta^(t+1))
  adam_scalars(lr_c, a.pow4[0], a.pow4[1], ss_c, bc2s_c);
  for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < a.P; i += (int64_t)gridDim.x * 256) {
    const bool act = i >= a.actor_begin;
    const AdamOut o = adam1(a.theta[i], a.grad[i] * coef, a.m[i], a.v[i], a.b2, a.w1, a.w2, a.eps, act ? ss_a : ss_c, act ? bc2s_a : bc2s_c);
    a.theta[i] = o.p; a.m[i] = o.m; a.v[i] = o.v;
  }
  // what wide_coef_kernel's single lane wrote besides the clocks: nobody else in this launch reads any of it
  if (blockIdx.x == 0 && tid == 0) {
    a.scal[0] = sh[0]; a.scal[1] = sh[1]; a.scal[2] = sh[2]; a.scal[3] = sh[3];
    const float l0 = a.losses3[0] + sh[1], l1 = a.losses3[1] + sh[2], l2v = a.losses3[2];   // logged critic losses include their L2 terms
    a.losses3[0] = l0; a.losses3[1] = l1;
    if (a.cursor && a.loss_log) {
      const int64_t at = a.cursor[0] - a.cursor_step;               // (the step's position: the cursor moved on in the pass in front)
      float* row = a.loss_log + 3 * (at / a.cursor_step);
      row[0] = l0; row[1] = l1; row[2] = l2v;
    }
  }
}

bool mr_enabled() {
  static const bool on = [] { const char* e = getenv("SPO_WIDE_ROWS"); return !(e && e[0] == '0'); }();
  return on;
}
int mr_fill_net(const spo_mlp_net* net, int64_t off, int kind, MrNet* o) {
  o->n = net->n_layers; o->kind = kind; o->poff = 0;
  for (int k = 0; k <= o->n; ++k) o->d[k] = net->dims[k];
  for (int l = 0; l < o->n; ++l) {
    o->w[l] = off; off += (int64_t)o->d[l + 1] * o->d[l];
    o->b[l] = off; off += o->d[l + 1];
  }
  for (int v = 0; v <= o->n; ++v) {
    const MrLevel L = mr_level(*o, v);
    o->pr[v] = L.pr; o->hr[v] = L.hr; o->ht[v] = L.ht;
  }
  o->pz = mr_pz(*o); o->zbase = mr_images_end(*o);
  return 0;
}
bool mr_net_ok(const spo_mlp_net* net, int A) {
  if (!net || net->n_layers < 1 || net->n_layers > SPO_MLP_MAX_LAYERS) return false;
  for (int k = 0; k <= net->n_layers; ++k)
    if (net->dims[k] < 1) return false;
  MrNet t;
  mr_fill_net(net, 0, 0, &t);
  return (size_t)mr_lds_floats(t, A) * sizeof(float) <= MR_MAX_LDS;
}
int64_t mr_stride(int64_t P) { return (P + 4 + 3) & ~(int64_t)3; }
// the KL-penalty launch's part of one row group: the gradient and eight row-sum slots, then the actor's policy-gradient part
int64_t mr_kl_pgoff(int64_t P) { return (P + 8 + 3) & ~(int64_t)3; }
int64_t mr_kl_stride(int64_t P, int64_t ab) { return mr_kl_pgoff(P) + ((P - ab + 3) & ~(int64_t)3); }
// LDS of the KL-penalty launch: the images of the wider of the two networks, and the old distribution behind the actor's
size_t mr_kl_lds_floats(const MrNet& critic, const MrNet& actor, int A) {
  const size_t lc = (size_t)mr_lds_floats(critic, A), la = (size_t)mr_lds_floats(actor, A) + (size_t)mr_klx(mr_ap(A));
  return la > lc ? la : lc;
}
// ---- the arguments of the fused PPO step's three launches, filled in ONE place for the stand-alone entries
// (spo_wide_ppo_grad_rows, spo_wide_rows_clip_adam_dev_log) and for every run of a seed-batched table (spo_wide_rows_multi_upload):
// run r of a table gets its stand-alone launch's arguments by construction.  No checks here: the callers made them.
void mr_fill_grad(const float* theta, const spo_mlp_net* critic, const spo_mlp_net* actor, const float* obs, const float* act,
                  const float* logp_old, const float* target_r, const float* target_c, const float* adv, const int64_t* idx,
                  const int64_t* cursor_dev, int64_t rows, float clip, float* parts, MrArgs* out, size_t* lds_bytes, bool* vec_out) {
  MrArgs& a = *out;
  a = MrArgs{};
  a.theta = theta; a.obs = obs; a.act = act; a.logp_old = logp_old; a.tgt_r = target_r; a.tgt_c = target_c; a.adv = adv;
  a.idx = idx; a.cursor = cursor_dev; a.rows = (int)rows; a.R = (int)((rows + 15) / 16); a.clip = clip;
  const int64_t Pc = spo_mlp_param_count(critic);
  mr_fill_net(critic, 0, 0, &a.net[0]);
  mr_fill_net(critic, Pc, 1, &a.net[1]);
  a.n_nets = 2; a.P = 2 * Pc; a.A = 0; a.ls_off = 2 * Pc;
  const int A_launch = actor ? actor->dims[actor->n_layers] : 0;
  size_t lds_floats = (size_t)mr_lds_floats(a.net[0], A_launch);
  if (actor) {
    a.A = actor->dims[actor->n_layers];
    mr_fill_net(actor, 2 * Pc + a.A, 2, &a.net[2]);
    a.n_nets = 3; a.P = 2 * Pc + a.A + spo_mlp_param_count(actor);
    const size_t la = (size_t)mr_lds_floats(a.net[2], A_launch);
    lds_floats = la > lds_floats ? la : lds_floats;
  }
  a.parts = parts; a.stride = mr_stride(a.P);
  *lds_bytes = lds_floats * sizeof(float);
  bool vec = true;                                   // every weight row a whole number of 16-byte fragments
  for (int k = 0; k < a.n_nets; ++k)
    for (int l = 0; l < a.net[k].n; ++l) vec = vec && (a.net[k].d[l] & 3) == 0;
  *vec_out = vec;
}
// the dynamic-LDS limit of the four PPO gradient kernels (stand-alone and table-driven), raised once per device
int mr_grad_attr_once() {
  static bool done_dev[SPO_MAX_DEVICES] = {};
  bool& done = done_dev[spo::current_device_slot()];
  if (!done) {
    for (const void* f : {reinterpret_cast<const void*>(&mlp_rows_grad_kernel<true>), reinterpret_cast<const void*>(&mlp_rows_grad_kernel<false>),
                          reinterpret_cast<const void*>(&mlp_rows_grad_kernel<true, MR_PPO, true>),
                          reinterpret_cast<const void*>(&mlp_rows_grad_kernel<false, MR_PPO, true>)})
      if (int rc = spo::hip_check(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MR_MAX_LDS),
                                  "hipFuncSetAttribute(mlp_rows)"))
        return rc;
    done = true;
  }
  return 0;
}
// ---- the same for the KL-penalty step's gradient launch and both group sums: the stand-alone entries
// (spo_wide_kl_penalty_grad_rows, spo_wide_kl_penalty_reduce_parts, spo_wide_reduce_parts) and every run of a seed-batched table
// (spo_wide_rows_ex_multi_upload) get their kernel arguments here.  No checks: the callers made them.
void mr_fill_klgrad(const float* theta, const spo_mlp_net* critic, const spo_mlp_net* actor, const float* obs, const float* act,
                    const float* logp_old, const float* target_r, const float* target_c, const float* adv, const float* old_mean,
                    const float* old_std, const int64_t* idx, const int64_t* cursor_dev, int64_t rows, float kl_bound, float pg_coef,
                    int actor_only, float* parts, MrArgs* out, size_t* lds_bytes, bool* vec_out) {
  MrArgs& a = *out;
  a = MrArgs{};
  a.theta = theta; a.obs = obs; a.act = act; a.logp_old = logp_old; a.tgt_r = target_r; a.tgt_c = target_c; a.adv = adv;
  a.old_mean = old_mean; a.old_std = old_std; a.kl_bound = kl_bound; a.pg_coef = pg_coef;
  a.idx = idx; a.cursor = cursor_dev; a.rows = (int)rows; a.R = (int)((rows + 15) / 16);
  const int64_t Pc = spo_mlp_param_count(critic);
  a.A = actor->dims[actor->n_layers];
  a.ls_off = 2 * Pc;
  a.P = 2 * Pc + a.A + spo_mlp_param_count(actor);
  a.parts = parts; a.stride = mr_kl_stride(a.P, a.ls_off);
  int k = 0;
  if (!actor_only) {
    mr_fill_net(critic, 0, 0, &a.net[k++]);
    mr_fill_net(critic, Pc, 1, &a.net[k++]);
  }
  mr_fill_net(actor, 2 * Pc + a.A, 2, &a.net[k++]);
  mr_fill_net(actor, 2 * Pc + a.A, 3, &a.net[k]);
  a.net[k].poff = mr_kl_pgoff(a.P) - a.ls_off;         // g_PG[i - actor_begin] behind the group's gradient and row sums
  a.n_nets = k + 1;
  MrNet c0;
  mr_fill_net(critic, 0, 0, &c0);
  *lds_bytes = mr_kl_lds_floats(c0, a.net[k], a.A) * sizeof(float);
  bool vec = true;
  for (int i = 0; i < a.n_nets; ++i)
    for (int l = 0; l < a.net[i].n; ++l) vec = vec && (a.net[i].d[l] & 3) == 0;
  *vec_out = vec;
}
// the dynamic-LDS limit of the four KL-penalty gradient kernels (stand-alone and table-driven), raised once per device
int mr_klgrad_attr_once() {
  static bool done_dev[SPO_MAX_DEVICES] = {};
  bool& done = done_dev[spo::current_device_slot()];
  if (!done) {
    for (const void* f : {reinterpret_cast<const void*>(&mlp_rows_grad_kernel<true, MR_KLPEN>),
                          reinterpret_cast<const void*>(&mlp_rows_grad_kernel<false, MR_KLPEN>),
                          reinterpret_cast<const void*>(&mlp_rows_grad_kernel<true, MR_KLPEN, true>),
                          reinterpret_cast<const void*>(&mlp_rows_grad_kernel<false, MR_KLPEN, true>)})
      if (int rc = spo::hip_check(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MR_MAX_LDS),
                                  "hipFuncSetAttribute(mlp_rows, KL penalty)"))
        return rc;
    done = true;
  }
  return 0;
}
// (both return the launch's workgroups)
int64_t mr_fill_klreduce(const float* parts, int64_t rows, int64_t n_params, int64_t actor_begin, int actor_only, int combine, float pg_coef,
                         float* grad, float* pg_grad, float* sums, float* losses_out, MrKlReduceArgs* out) {
  const int64_t lo = actor_only ? actor_begin : 0;
  *out = MrKlReduceArgs{parts, (int)((rows + 15) / 16), mr_kl_stride(n_params, actor_begin), n_params, actor_begin, lo, mr_kl_pgoff(n_params),
                        rows, actor_only ? 0 : 2, combine, pg_coef, grad, pg_grad, sums, losses_out};
  const int64_t blocks = (n_params - lo + 255) / 256;
  return blocks > 512 ? 512 : (blocks < 1 ? 1 : blocks);
}
int64_t mr_fill_reduce(const float* parts, int64_t rows, int64_t n_params, int n_losses, float* grad, float* losses_out, MrReduceArgs* out) {
  *out = MrReduceArgs{parts, (int)((rows + 15) / 16), mr_stride(n_params), n_params, rows, n_losses, grad, losses_out};
  const int64_t blocks = (n_params + 255) / 256;
  return blocks > 512 ? 512 : blocks;
}
int64_t mr_opt_blocks(int64_t n_params) {
  const int64_t blocks = (n_params + 255) / 256;
  return blocks > 1024 ? 1024 : blocks;
}
// the optimiser launches' refusals behind the null-pointer check, worded with the entry's name (`who`)
int mr_check_ranges(const char* who, int64_t n_params, int64_t reward_critic_end, int64_t cost_critic_end, int64_t actor_begin) {
  SPO_REQUIRE(0 <= reward_critic_end && reward_critic_end <= cost_critic_end && cost_critic_end <= actor_begin && actor_begin <= n_params,
              "%s: parameter ranges out of order", who);
  return 0;
}
int mr_check_partial(const char* who, int64_t n_params, int partial_capacity) {
  SPO_REQUIRE((int64_t)partial_capacity >= mr_opt_blocks(n_params) * 3, "%s: partial workspace too small", who);
  return 0;
}
int mr_fill_opt(const char* who, float* parts, int64_t rows, float* theta, float* grad, float* adam_m, float* adam_v, int64_t n_params,
                 int64_t reward_critic_end, int64_t cost_critic_end, int64_t actor_begin, const spo_ppo_cfg* cfg, double* pow4_dev,
                 float* losses3_out, float* scalars4_out, double* partial_ws, float* loss_log_dev, int64_t* cursor_dev,
                 int64_t cursor_step, MrOptArgs* out) {
  const int R = (int)((rows + 15) / 16);
  const int64_t stride = mr_stride(n_params);
  float w1, w2;
  double b1d = 0.0, b2d = 0.0;
  SPO_REQUIRE(adam_beta_host(cfg->beta1, &b1d, &w1) && adam_beta_host(cfg->beta2, &b2d, &w2), "%s: betas (%g, %g) outside [0, 1)", who,
              (double)cfg->beta1, (double)cfg->beta2);
  *out = MrOptArgs{parts, R, stride, theta, grad, adam_m, adam_v, n_params, reward_critic_end, cost_critic_end, actor_begin, rows,
                   cfg->use_critic_norm ? cfg->l2_coef : 0.f, cfg->use_value_coefficient ? 2.f : 1.f, cfg->max_grad_norm, cfg->lr_actor,
                   cfg->lr_critic, cfg->beta1, cfg->beta2, cfg->adam_eps, w1, w2, b1d, b2d, partial_ws, scalars4_out, losses3_out, pow4_dev, loss_log_dev,
                   cursor_dev, cursor_step, (int)mr_opt_blocks(n_params)};
  return 0;
}
}  // namespace

#ifdef SPO_MR_PROF
extern "C" int spo_debug_mr_profile(unsigned long long* out64_host) {
  return spo::hip_check(hipMemcpyFromSymbol(out64_host, HIP_SYMBOL(g_mr_prof), sizeof(unsigned long long) * 64), "mr_prof");
}
#endif

extern "C" int spo_wide_grad_rows_supported(const spo_mlp_net* critic, const spo_mlp_net* actor, int64_t rows) {
  if (!mr_enabled() || rows < 1 || rows > 16 * MR_MAX_GROUPS) return 0;
  if (!critic || critic->n_layers < 1 || critic->n_layers > SPO_MLP_MAX_LAYERS || critic->dims[critic->n_layers] != 1) return 0;
  if (actor && (actor->n_layers < 1 || actor->n_layers > SPO_MLP_MAX_LAYERS || actor->dims[0] != critic->dims[0] ||
                actor->dims[actor->n_layers] < 1 || actor->dims[actor->n_layers] > SPO_WIDE_MAX_ACT))
    return 0;
  const int A = actor ? actor->dims[actor->n_layers] : 0;
  if (!mr_net_ok(critic, A) || (actor && !mr_net_ok(actor, A))) return 0;
  return 1;
}

extern "C" int64_t spo_wide_grad_rows_part_floats(int64_t n_params, int64_t rows) {
  if (n_params < 1 || rows < 1) return -1;
  return ((rows + 15) / 16) * mr_stride(n_params) + 4;
}

// n_nets = 3: reward critic, cost critic, actor (theta = [critic | critic | log_std | actor], the ActorVCritic layout of
// safepo/common/wide.py); n_nets = 2: the two critics only (the critic fit of the second-order scripts, cpo.py:541-556).
extern "C" int spo_wide_ppo_grad_rows(const float* theta, const spo_mlp_net* critic, const spo_mlp_net* actor, const float* obs,
                                      const float* act, const float* logp_old, const float* target_r, const float* target_c,
                                      const float* adv, const int64_t* idx, const int64_t* cursor_dev, int64_t rows, float clip,
                                      float* parts, void* stream) {
  SPO_REQUIRE(theta && critic && obs && target_r && target_c && parts, "wide_ppo_grad_rows: null pointer");
  SPO_REQUIRE(!actor || (act && logp_old && adv), "wide_ppo_grad_rows: the actor needs act / logp_old / adv");
  SPO_REQUIRE(spo_wide_grad_rows_supported(critic, actor, rows), "wide_ppo_grad_rows: shape outside the row-group kernel (rows %lld)",
              (long long)rows);
  MrArgs a{};
  size_t sh = 0;
  bool vec = true;
  mr_fill_grad(theta, critic, actor, obs, act, logp_old, target_r, target_c, adv, idx, cursor_dev, rows, clip, parts, &a, &sh, &vec);
  hipStream_t st = (hipStream_t)stream;
  if (int rc = mr_grad_attr_once()) return rc;
  if (vec) hipLaunchKernelGGL(mlp_rows_grad_kernel<true>, dim3(a.n_nets * a.R), dim3(512), sh, st, a);
  else hipLaunchKernelGGL(mlp_rows_grad_kernel<false>, dim3(a.n_nets * a.R), dim3(512), sh, st, a);
  SPO_LAUNCH_CHECK("spo_wide_ppo_grad_rows");
  return 0;
}

// grad[0 .. n_params) = the sum of the row groups' partial gradients, losses_out[0 .. n_losses) = the data losses
// {MSE reward critic, MSE cost critic, clipped surrogate} of the `rows`-row minibatch (n_losses 2: the critics only).
extern "C" int spo_wide_reduce_parts(const float* parts, int64_t rows, int64_t n_params, int n_losses, float* grad, float* losses_out,
                                     void* stream) {
  SPO_REQUIRE(parts && grad && rows >= 1 && rows <= 16 * MR_MAX_GROUPS && n_params >= 1 && n_losses >= 0 && n_losses <= 3,
              "wide_reduce_parts: bad args");
  MrReduceArgs a;
  const int64_t blocks = mr_fill_reduce(parts, rows, n_params, n_losses, grad, losses_out, &a);
  hipLaunchKernelGGL(mlp_rows_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a.parts, a.R, a.stride, a.P, a.rows,
                     a.n_loss, a.grad, a.losses);
  SPO_LAUNCH_CHECK("spo_wide_reduce_parts");
  return 0;
}

// spo_wide_reduce_parts + spo_wide_clip_adam_dev_log (full ranges: the PPO-Lagrangian step, ppo_lag.py:310-329) in two launches --
// see mlp_rows_prep_kernel / mlp_rows_adam_kernel.  parts: the buffer spo_wide_ppo_grad_rows filled.  grad receives the clipped step's
// pre-clip gradient (with the L2 terms), losses3_out the step's losses, pow4_dev / cursor_dev advance as in
// spo_wide_clip_adam_dev_log (loss_log_dev row = the three losses).
extern "C" int spo_wide_rows_clip_adam_dev_log(float* parts, int64_t rows, float* theta, float* grad, float* adam_m, float* adam_v,
                                               int64_t n_params, int64_t reward_critic_end, int64_t cost_critic_end,
                                               int64_t actor_begin, const spo_ppo_cfg* cfg, double* pow4_dev, float* losses3_out,
                                               float* scalars4_out, double* partial_ws, int partial_capacity, float* loss_log_dev,
                                               int64_t* cursor_dev, int64_t cursor_step, void* stream) {
  SPO_REQUIRE(parts && theta && grad && adam_m && adam_v && cfg && pow4_dev && losses3_out && scalars4_out && partial_ws && n_params > 0 &&
                  rows >= 1 && rows <= 16 * MR_MAX_GROUPS, "wide_rows_clip_adam: bad args");
  if (int rc = mr_check_ranges("wide_rows_clip_adam", n_params, reward_critic_end, cost_critic_end, actor_begin)) return rc;
  SPO_REQUIRE(!cursor_dev || cursor_step > 0, "wide_rows_clip_adam: cursor_step must be > 0");
  if (int rc = mr_check_partial("wide_rows_clip_adam", n_params, partial_capacity)) return rc;
  const int64_t blocks = mr_opt_blocks(n_params);
  MrOptArgs a;
  if (int rc = mr_fill_opt("wide_rows_clip_adam", parts, rows, theta, grad, adam_m, adam_v, n_params, reward_critic_end, cost_critic_end,
                           actor_begin, cfg, pow4_dev, losses3_out, scalars4_out, partial_ws, loss_log_dev, cursor_dev, cursor_step, &a))
    return rc;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mlp_rows_prep_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, a);
  hipLaunchKernelGGL(mlp_rows_adam_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, a);
  SPO_LAUNCH_CHECK("spo_wide_rows_clip_adam_dev_log");
  return 0;
}

// ---- the seed-batched fused PPO step: S runs of one shape in the stand-alone step's three launches (include/safepo_hip.h)
extern "C" int spo_wide_rows_multi_supported(const spo_mlp_net* critic, const spo_mlp_net* actor, int64_t rows, int n_replicas) {
  if (!actor || n_replicas < 1 || n_replicas > SPO_WIDE_ROWS_MAX_REPLICAS) return 0;
  return spo_wide_grad_rows_supported(critic, actor, rows);
}

extern "C" int64_t spo_wide_rows_multi_table_bytes(int n_replicas) {
  if (n_replicas < 1 || n_replicas > SPO_WIDE_ROWS_MAX_REPLICAS) return -1;
  return (int64_t)n_replicas * (int64_t)sizeof(MrMultiEntry);
}

extern "C" int spo_wide_rows_multi_upload(void* table_dev, const spo_wide_rows_replica* reps_host, int n_replicas,
                                          const spo_mlp_net* critic, const spo_mlp_net* actor, int64_t rows, int64_t cursor_step,
                                          void* stream) {
  SPO_REQUIRE(table_dev && reps_host, "wide_rows_multi_upload: null table");
  SPO_REQUIRE(n_replicas >= 1 && n_replicas <= SPO_WIDE_ROWS_MAX_REPLICAS, "wide_rows_multi_upload: n_replicas %d outside [1,%d]",
              n_replicas, SPO_WIDE_ROWS_MAX_REPLICAS);
  SPO_REQUIRE(spo_wide_rows_multi_supported(critic, actor, rows, n_replicas),
              "wide_rows_multi_upload: shape outside the row-group kernel (rows %lld)", (long long)rows);
  for (int r = 0; r < n_replicas; ++r) {
    const spo_wide_rows_replica& p = reps_host[r];
    SPO_REQUIRE(!p.active || (p.theta && p.adam_m && p.adam_v && p.grad && p.parts && p.obs && p.act && p.logp_old && p.target_r &&
                              p.target_c && p.adv && p.perm && p.cursor_dev && p.pow4_dev && p.losses3_out && p.scalars4_out &&
                              p.partial_ws),
                "wide_rows_multi_upload: replica %d: null pointer", r);
  }
  for (int r = 0; r < n_replicas; ++r)
    for (int q = 0; q < r; ++q) {
      const spo_wide_rows_replica &x = reps_host[q], &y = reps_host[r];
      if (!x.active || !y.active) continue;
      SPO_REQUIRE(x.theta != y.theta, "wide_rows_multi_upload: replicas %d and %d share theta", q, r);
      SPO_REQUIRE(x.parts != y.parts, "wide_rows_multi_upload: replicas %d and %d share parts", q, r);
      SPO_REQUIRE(x.cursor_dev != y.cursor_dev, "wide_rows_multi_upload: replicas %d and %d share cursor_dev", q, r);
    }
  const int64_t Pc = spo_mlp_param_count(critic);
  const int64_t P = 2 * Pc + actor->dims[actor->n_layers] + spo_mlp_param_count(actor);
  if (int rc = mr_check_ranges("wide_rows_multi_upload", P, Pc, 2 * Pc, 2 * Pc)) return rc;
  for (int r = 0; r < n_replicas; ++r)
    if (reps_host[r].active)
      if (int rc = mr_check_partial("wide_rows_multi_upload", P, reps_host[r].partial_capacity)) return rc;
  SPO_REQUIRE(cursor_step > 0, "wide_rows_multi_upload: cursor_step must be > 0");
  // (the entries of inactive runs stay zero: their blocks read `active` and nothing else)
  static thread_local std::vector<MrMultiEntry> tab;
  tab.assign((size_t)n_replicas, MrMultiEntry{});
  for (int r = 0; r < n_replicas; ++r) {
    const spo_wide_rows_replica& p = reps_host[r];
    if (!p.active) continue;
    MrMultiEntry& e = tab[(size_t)r];
    size_t sh;
    bool vec;
    mr_fill_grad(p.theta, critic, actor, p.obs, p.act, p.logp_old, p.target_r, p.target_c, p.adv, p.perm, p.cursor_dev, rows,
                 p.cfg.clip, p.parts, &e.g, &sh, &vec);
    if (int rc = mr_fill_opt("wide_rows_multi_upload", p.parts, rows, p.theta, p.grad, p.adam_m, p.adam_v, P, Pc, 2 * Pc, 2 * Pc, &p.cfg,
                             p.pow4_dev, p.losses3_out, p.scalars4_out, p.partial_ws, p.loss_log_dev, p.cursor_dev, cursor_step, &e.o))
      return rc;
    e.active = 1;
  }
  hipStream_t st = (hipStream_t)stream;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
    return spo::fail(-1, "wide_rows_multi_upload: the stream is under capture (the argument table is copied from host memory: "
                         "upload outside the capture, capture spo_wide_rows_step_multi)");
  // stream-ordered behind the replays that still read the previous table; the host table is reused by the next call: wait
  if (int rc = spo::hip_check(hipMemcpyAsync(table_dev, tab.data(), (size_t)n_replicas * sizeof(MrMultiEntry), hipMemcpyHostToDevice, st),
                              "hipMemcpyAsync(wide_rows_multi table)"))
    return rc;
  return spo::hip_check(hipStreamSynchronize(st), "hipStreamSynchronize(wide_rows_multi table)");
}

extern "C" int spo_wide_rows_step_multi(const void* table_dev, int n_replicas, const spo_mlp_net* critic, const spo_mlp_net* actor,
                                        int64_t rows, void* stream) {
  SPO_REQUIRE(table_dev, "wide_rows_step_multi: null table");
  SPO_REQUIRE(n_replicas >= 1 && n_replicas <= SPO_WIDE_ROWS_MAX_REPLICAS, "wide_rows_step_multi: n_replicas %d outside [1,%d]",
              n_replicas, SPO_WIDE_ROWS_MAX_REPLICAS);
  SPO_REQUIRE(spo_wide_rows_multi_supported(critic, actor, rows, n_replicas),
              "wide_rows_step_multi: shape outside the row-group kernel (rows %lld)", (long long)rows);
  // the launch shape of a run: what mr_fill_grad / mr_fill_opt give its stand-alone launches (pointers play no part in it)
  MrArgs a;
  size_t sh;
  bool vec;
  mr_fill_grad(nullptr, critic, actor, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, rows, 0.f, nullptr, &a, &sh,
               &vec);
  const unsigned blocks = (unsigned)mr_opt_blocks(a.P);
  const MrMultiEntry* tab = static_cast<const MrMultiEntry*>(table_dev);
  hipStream_t st = (hipStream_t)stream;
  if (int rc = mr_grad_attr_once()) return rc;
  const dim3 ggrid((unsigned)(a.n_nets * a.R), (unsigned)n_replicas), ogrid(blocks, (unsigned)n_replicas);
  if (vec) hipLaunchKernelGGL((mlp_rows_grad_kernel<true, MR_PPO, true>), ggrid, dim3(512), sh, st, tab);
  else hipLaunchKernelGGL((mlp_rows_grad_kernel<false, MR_PPO, true>), ggrid, dim3(512), sh, st, tab);
  hipLaunchKernelGGL(mlp_rows_prep_kernel<true>, ogrid, dim3(256), 0, st, tab);
  hipLaunchKernelGGL(mlp_rows_adam_kernel<true>, ogrid, dim3(256), 0, st, tab);
  SPO_LAUNCH_CHECK("spo_wide_rows_step_multi");
  return 0;
}

// ---- the KL-penalty loss of FOCOPS (focops.py:326-347) and CUP's second stage (cup.py:370-386) on the row groups
extern "C" int spo_wide_kl_penalty_grad_rows_supported(const spo_mlp_net* critic, const spo_mlp_net* actor, int64_t rows) {
  if (!actor || !spo_wide_grad_rows_supported(critic, actor, rows)) return 0;
  const int A = actor->dims[actor->n_layers];
  MrNet c, t;
  mr_fill_net(critic, 0, 0, &c);
  mr_fill_net(actor, 0, 2, &t);
  return mr_kl_lds_floats(c, t, A) * sizeof(float) <= MR_MAX_LDS ? 1 : 0;
}

extern "C" int64_t spo_wide_kl_penalty_rows_part_floats(int64_t n_params, int64_t actor_begin, int64_t rows) {
  if (n_params < 1 || rows < 1 || actor_begin < 0 || actor_begin > n_params) return -1;
  // (behind the groups: room for a pg_grad indexed like grad and the sums, for callers that only want the combined gradient)
  return ((rows + 15) / 16) * mr_kl_stride(n_params, actor_begin) + ((n_params + 3) & ~(int64_t)3) + SPO_KLPEN_SUMS + 4;
}

extern "C" int spo_wide_kl_penalty_grad_rows(const float* theta, const spo_mlp_net* critic, const spo_mlp_net* actor, const float* obs,
                                             const float* act, const float* logp_old, const float* target_r, const float* target_c,
                                             const float* adv, const float* old_mean, const float* old_std, const int64_t* idx,
                                             const int64_t* cursor_dev, int64_t rows, float kl_bound, float pg_coef, int actor_only,
                                             float* parts, void* stream) {
  SPO_REQUIRE(theta && critic && actor && obs && act && logp_old && adv && old_mean && old_std && parts,
              "wide_kl_penalty_grad_rows: null pointer");
  SPO_REQUIRE(actor_only || (target_r && target_c), "wide_kl_penalty_grad_rows: critic targets are NULL");
  SPO_REQUIRE(rows >= 1 && rows <= 16 * MR_MAX_GROUPS, "wide_kl_penalty_grad_rows: rows %lld outside [1,%d]", (long long)rows,
              16 * MR_MAX_GROUPS);
  SPO_REQUIRE(spo_wide_kl_penalty_grad_rows_supported(critic, actor, rows),
              "wide_kl_penalty_grad_rows: shape outside the row-group kernel (rows %lld)", (long long)rows);
  MrArgs a{};
  size_t sh = 0;
  bool vec = true;
  mr_fill_klgrad(theta, critic, actor, obs, act, logp_old, target_r, target_c, adv, old_mean, old_std, idx, cursor_dev, rows, kl_bound,
                 pg_coef, actor_only, parts, &a, &sh, &vec);
  hipStream_t st = (hipStream_t)stream;
  if (int rc = mr_klgrad_attr_once()) return rc;
  if (vec) hipLaunchKernelGGL((mlp_rows_grad_kernel<true, MR_KLPEN>), dim3(a.n_nets * a.R), dim3(512), sh, st, a);
  else hipLaunchKernelGGL((mlp_rows_grad_kernel<false, MR_KLPEN>), dim3(a.n_nets * a.R), dim3(512), sh, st, a);
  SPO_LAUNCH_CHECK("spo_wide_kl_penalty_grad_rows");
  return 0;
}

extern "C" int spo_wide_kl_penalty_reduce_parts(const float* parts, int64_t rows, int64_t n_params, int64_t actor_begin, int actor_only,
                                                int combine, float pg_coef, float* grad, float* pg_grad, float* sums, float* losses_out,
                                                void* stream) {
  SPO_REQUIRE(parts && grad && pg_grad && sums, "wide_kl_penalty_reduce_parts: null pointer");
  SPO_REQUIRE(rows >= 1 && rows <= 16 * MR_MAX_GROUPS && n_params >= 1 && actor_begin >= 0 && actor_begin <= n_params,
              "wide_kl_penalty_reduce_parts: bad args (rows %lld, n_params %lld, actor_begin %lld)", (long long)rows, (long long)n_params,
              (long long)actor_begin);
  MrKlReduceArgs a;
  const int64_t blocks = mr_fill_klreduce(parts, rows, n_params, actor_begin, actor_only, combine, pg_coef, grad, pg_grad, sums, losses_out, &a);
  hipLaunchKernelGGL(mlp_rows_klpen_reduce_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  SPO_LAUNCH_CHECK("spo_wide_kl_penalty_reduce_parts");
  return 0;
}

// ---- the seed-batched FOCOPS / CUP step: S runs of one shape in the stand-alone step's five launches (include/safepo_hip.h).
// The device table: [S x MrMultiEntry] (the gradient launch: g and active; o stays zero) | [S x MrRedEntry] (the group sum) |
// [S x csrc/wide_opt.h's entry] (prep, coefficient, Adam), each block 16-byte aligned.
namespace {
struct MrExLayout { size_t off_red, off_opt, bytes; };
MrExLayout mr_ex_layout(int S) {
  const auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
  MrExLayout L;
  L.off_red = up16((size_t)S * sizeof(MrMultiEntry));
  L.off_opt = L.off_red + up16((size_t)S * sizeof(MrRedEntry));
  L.bytes = L.off_opt + (size_t)S * spo::wide_opt_entry_bytes();
  return L;
}
bool mr_ex_kind_ok(int actor_loss, int actor_only) {
  return (actor_loss == SPO_ACTOR_LOSS_CLIP && !actor_only) || actor_loss == SPO_ACTOR_LOSS_KL_PENALTY;
}
}  // namespace

extern "C" int spo_wide_rows_ex_multi_supported(const spo_mlp_net* critic, const spo_mlp_net* actor, int64_t rows, int actor_loss,
                                                int actor_only, int n_replicas) {
  if (!actor || n_replicas < 1 || n_replicas > SPO_WIDE_ROWS_MAX_REPLICAS || !mr_ex_kind_ok(actor_loss, actor_only)) return 0;
  return actor_loss == SPO_ACTOR_LOSS_KL_PENALTY ? spo_wide_kl_penalty_grad_rows_supported(critic, actor, rows)
                                                 : spo_wide_grad_rows_supported(critic, actor, rows);
}

extern "C" int64_t spo_wide_rows_ex_multi_table_bytes(int n_replicas) {
  if (n_replicas < 1 || n_replicas > SPO_WIDE_ROWS_MAX_REPLICAS) return -1;
  return (int64_t)mr_ex_layout(n_replicas).bytes;
}

extern "C" int spo_wide_rows_ex_multi_upload(void* table_dev, const spo_wide_rows_ex_replica* reps_host, int n_replicas,
                                             const spo_mlp_net* critic, const spo_mlp_net* actor, int64_t rows, int64_t cursor_step,
                                             int actor_loss, int actor_only, void* stream) {
  const bool klpen = actor_loss == SPO_ACTOR_LOSS_KL_PENALTY;
  SPO_REQUIRE(table_dev && reps_host, "wide_rows_ex_multi_upload: null table");
  SPO_REQUIRE(n_replicas >= 1 && n_replicas <= SPO_WIDE_ROWS_MAX_REPLICAS, "wide_rows_ex_multi_upload: n_replicas %d outside [1,%d]",
              n_replicas, SPO_WIDE_ROWS_MAX_REPLICAS);
  SPO_REQUIRE(actor_loss == SPO_ACTOR_LOSS_CLIP || klpen, "wide_rows_ex_multi_upload: actor_loss %d is neither SPO_ACTOR_LOSS_CLIP nor "
              "SPO_ACTOR_LOSS_KL_PENALTY", actor_loss);
  SPO_REQUIRE(mr_ex_kind_ok(actor_loss, actor_only), "wide_rows_ex_multi_upload: actor_only needs the KL-penalty loss (the clipped "
              "surrogate's step takes the critics along)");
  SPO_REQUIRE(spo_wide_rows_ex_multi_supported(critic, actor, rows, actor_loss, actor_only, n_replicas),
              "wide_rows_ex_multi_upload: shape outside the row-group kernel's %s form (rows %lld)", klpen ? "KL-penalty" : "clipped-surrogate",
              (long long)rows);
  for (int r = 0; r < n_replicas; ++r) {
    const spo_wide_rows_ex_replica& p = reps_host[r];
    SPO_REQUIRE(!p.active || (p.theta && p.adam_m && p.adam_v && p.grad && p.parts && p.obs && p.act && p.logp_old && p.adv && p.perm &&
                              p.cursor_dev && p.pow4_dev && p.losses3_out && p.scalars4_out && p.partial_ws),
                "wide_rows_ex_multi_upload: replica %d: null pointer", r);
    SPO_REQUIRE(!p.active || actor_only || (p.target_r && p.target_c), "wide_rows_ex_multi_upload: replica %d: critic targets are NULL", r);
    SPO_REQUIRE(!p.active || !klpen || (p.old_mean && p.old_std), "wide_rows_ex_multi_upload: replica %d: the KL-penalty loss needs "
                "old_mean / old_std", r);
  }
  for (int r = 0; r < n_replicas; ++r)
    for (int q = 0; q < r; ++q) {
      const spo_wide_rows_ex_replica &x = reps_host[q], &y = reps_host[r];
      if (!x.active || !y.active) continue;
      SPO_REQUIRE(x.theta != y.theta, "wide_rows_ex_multi_upload: replicas %d and %d share theta", q, r);
      SPO_REQUIRE(x.parts != y.parts, "wide_rows_ex_multi_upload: replicas %d and %d share parts", q, r);
      SPO_REQUIRE(x.cursor_dev != y.cursor_dev, "wide_rows_ex_multi_upload: replicas %d and %d share cursor_dev", q, r);
    }
  SPO_REQUIRE(cursor_step > 0, "wide_rows_ex_multi_upload: cursor_step must be > 0");
  const int64_t Pc = spo_mlp_param_count(critic);
  const int64_t off_ls = 2 * Pc, P = off_ls + actor->dims[actor->n_layers] + spo_mlp_param_count(actor);
  const int64_t lo = actor_only ? off_ls : 0;                      // CUP's second stage: the actor's range in the norm and in Adam
  const int R = (int)((rows + 15) / 16);
  // (the entries of inactive runs stay zero: their blocks read `active` and nothing else)
  const MrExLayout L = mr_ex_layout(n_replicas);
  static thread_local std::vector<unsigned char> tab;
  tab.assign(L.bytes, 0);
  MrMultiEntry* const tg = reinterpret_cast<MrMultiEntry*>(tab.data());
  MrRedEntry* const tr = reinterpret_cast<MrRedEntry*>(tab.data() + L.off_red);
  for (int r = 0; r < n_replicas; ++r) {
    const spo_wide_rows_ex_replica& p = reps_host[r];
    if (!p.active) continue;
    size_t sh;
    bool vec;
    if (klpen) {
      mr_fill_klgrad(p.theta, critic, actor, p.obs, p.act, p.logp_old, p.target_r, p.target_c, p.adv, p.old_mean, p.old_std, p.perm,
                     p.cursor_dev, rows, p.kl_bound, p.pg_coef, actor_only, p.parts, &tg[r].g, &sh, &vec);
      // pg_grad / sums: the tail of `parts` behind the row groups (spo_wide_kl_penalty_rows_part_floats)
      float* const pg = p.parts + (int64_t)R * mr_kl_stride(P, off_ls);
      mr_fill_klreduce(p.parts, rows, P, off_ls, actor_only, 1, p.pg_coef, p.grad, pg, pg + ((P + 3) & ~(int64_t)3), p.losses3_out, &tr[r].kr);
    } else {
      mr_fill_grad(p.theta, critic, actor, p.obs, p.act, p.logp_old, p.target_r, p.target_c, p.adv, p.perm, p.cursor_dev, rows,
                   p.cfg.clip, p.parts, &tg[r].g, &sh, &vec);
      mr_fill_reduce(p.parts, rows, P, 3, p.grad, p.losses3_out, &tr[r].r);
    }
    if (int rc = spo::wide_opt_fill("wide_rows_ex_multi_upload", tab.data() + L.off_opt + (size_t)r * spo::wide_opt_entry_bytes(), p.theta,
                                    p.grad, p.adam_m, p.adam_v, P, Pc, off_ls, off_ls, &p.cfg, p.pow4_dev, lo, P, lo, 0,
                                    actor_only ? nullptr : p.losses3_out, p.scalars4_out, p.partial_ws, p.partial_capacity,
                                    p.loss_log_dev, p.losses3_out, p.cursor_dev, cursor_step))
      return rc;
    tg[r].active = 1;
    tr[r].active = 1;
  }
  hipStream_t st = (hipStream_t)stream;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
    return spo::fail(-1, "wide_rows_ex_multi_upload: the stream is under capture (the argument table is copied from host memory: "
                         "upload outside the capture, capture spo_wide_rows_ex_step_multi)");
  // stream-ordered behind the replays that still read the previous table; the host table is reused by the next call: wait
  if (int rc = spo::hip_check(hipMemcpyAsync(table_dev, tab.data(), L.bytes, hipMemcpyHostToDevice, st),
                              "hipMemcpyAsync(wide_rows_ex_multi table)"))
    return rc;
  return spo::hip_check(hipStreamSynchronize(st), "hipStreamSynchronize(wide_rows_ex_multi table)");
}

extern "C" int spo_wide_rows_ex_step_multi(const void* table_dev, int n_replicas, const spo_mlp_net* critic, const spo_mlp_net* actor,
                                           int64_t rows, int actor_loss, int actor_only, void* stream) {
  const bool klpen = actor_loss == SPO_ACTOR_LOSS_KL_PENALTY;
  SPO_REQUIRE(table_dev, "wide_rows_ex_step_multi: null table");
  SPO_REQUIRE(n_replicas >= 1 && n_replicas <= SPO_WIDE_ROWS_MAX_REPLICAS, "wide_rows_ex_step_multi: n_replicas %d outside [1,%d]",
              n_replicas, SPO_WIDE_ROWS_MAX_REPLICAS);
  SPO_REQUIRE(spo_wide_rows_ex_multi_supported(critic, actor, rows, actor_loss, actor_only, n_replicas),
              "wide_rows_ex_step_multi: shape or loss outside the row-group kernel (rows %lld, actor_loss %d, actor_only %d)", (long long)rows,
              actor_loss, actor_only);
  // the launch shape of a run: what the fillers give its stand-alone launches (pointers play no part in it)
  MrArgs a;
  MrKlReduceArgs kr;
  MrReduceArgs rr;
  size_t sh;
  bool vec;
  int64_t rblocks;
  if (klpen) {
    mr_fill_klgrad(nullptr, critic, actor, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, rows,
                   0.f, 0.f, actor_only, nullptr, &a, &sh, &vec);
    rblocks = mr_fill_klreduce(nullptr, rows, a.P, a.ls_off, actor_only, 1, 0.f, nullptr, nullptr, nullptr, nullptr, &kr);
  } else {
    mr_fill_grad(nullptr, critic, actor, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, rows, 0.f, nullptr, &a, &sh,
                 &vec);
    rblocks = mr_fill_reduce(nullptr, rows, a.P, 3, nullptr, nullptr, &rr);
  }
  const MrExLayout L = mr_ex_layout(n_replicas);
  const unsigned char* base = static_cast<const unsigned char*>(table_dev);
  const MrMultiEntry* tg = reinterpret_cast<const MrMultiEntry*>(base);
  const MrRedEntry* tr = reinterpret_cast<const MrRedEntry*>(base + L.off_red);
  hipStream_t st = (hipStream_t)stream;
  if (int rc = klpen ? mr_klgrad_attr_once() : mr_grad_attr_once()) return rc;
  const dim3 ggrid((unsigned)(a.n_nets * a.R), (unsigned)n_replicas), rgrid((unsigned)rblocks, (unsigned)n_replicas);
  if (klpen) {
    if (vec) hipLaunchKernelGGL((mlp_rows_grad_kernel<true, MR_KLPEN, true>), ggrid, dim3(512), sh, st, tg);
    else hipLaunchKernelGGL((mlp_rows_grad_kernel<false, MR_KLPEN, true>), ggrid, dim3(512), sh, st, tg);
    hipLaunchKernelGGL(mlp_rows_klpen_reduce_kernel<true>, rgrid, dim3(256), 0, st, tr);
  } else {
    if (vec) hipLaunchKernelGGL((mlp_rows_grad_kernel<true, MR_PPO, true>), ggrid, dim3(512), sh, st, tg);
    else hipLaunchKernelGGL((mlp_rows_grad_kernel<false, MR_PPO, true>), ggrid, dim3(512), sh, st, tg);
    hipLaunchKernelGGL(mlp_rows_reduce_multi_kernel, rgrid, dim3(256), 0, st, tr);
  }
  spo::wide_opt_launch_multi(base + L.off_opt, n_replicas, a.P, actor_only ? a.ls_off : 0, st);
  SPO_LAUNCH_CHECK("spo_wide_rows_ex_step_multi");
  return 0;
}
