// One candidate of MACPO's backtracking line search for the multi-agent actor, hidden width <= 128, gfx950 (spo_ma_ls_eval).
//
// Reference: safepo/multi_agent/macpo.py:329-366 evaluates up to `searching_steps` candidates theta_old - c x; for each one the
// host ran spo_ma_forward (input LayerNorm, fold, one or two launches per block, head: 5 launches at hidden 128 / two blocks, every
// activation of every row written to the workspace and never read) and then spo_ma_trpo_linesearch_sums (2 launches) or, in the
// host-driven form, spo_ma_log_probs and a dozen torch launches with three host reads.  Here a candidate is two launches:
// ma_ls_eval_kernel takes the raw observations through the network on chip and leaves one fp64 quadruple per workgroup,
// ma_ls_eval_reduce_kernel adds the quadruples in a fixed order.  Nothing but the four sums and the per-row ratio is written.
// Envelope (spo_ma_ls_eval_supported): the one of spo_ma_fvp -- an actor, in_dim 1..128, hidden 1..128, out_dim 1..16, 1 or 2 blocks.
//
// The network is  LayerNorm -> [Linear -> ELU -> LayerNorm] x NB -> Linear head  (ma_net.hip).  The input LayerNorm's affine is
// folded into block 0 as spo_ma_forward does, but without a launch or scratch: W'_0[n][c] = W_0[n][c] gamma[c] is formed on the
// A fragments as they are loaded, b'_0 = b_0 + W_0 beta once per workgroup into LDS (lane and summation order of fn_fold_kernel).
//
// Grid: at most 256 workgroups of 256 threads = 4 waves, each playing two of eight "virtual waves" (rows_frag.h); workgroup b walks
// the 32-row chunks b, b + gridDim, ...  Weights are read as v_mfma_f32_16x16x4_f32 (exact fp32) A fragments straight from global
// memory / L2.  LDS holds the chunk as ROW images [32][132]:
//
//   X            the normalised observations, zero beyond in_dim                              32 x 132
//   P[0], P[1]   block k's ELU values, then its LayerNorm output in place, in P[k & 1]        32 x 132 each
//   MU           the head's output                                                            32 x 20
//   BF, DC       b'_0 [128]; per action dimension std, std_old^2, log std_old - log std [3][16]
//   3 x 16 896 + 2 560 + 512 + 192 = 53 952 B for either block count.
//
// Sub-phases of one chunk, one barrier after each:
//   N          8 lanes per row load the raw observation row (float4 per lane where the alignment allows), normalise it in
//              registers (fixed-order lane sums xor 1, 2, 4; epsilon, mean and biased variance as the feature-norm kernels of
//              ma_net.hip) and write X -- the raw row never touches LDS
//   per block  T   ELU(b + W IN) on the feature-tile owners (tile w, both row tiles; hidden <= 64: tile w / 2, row tile w & 1)
//              L   the row LayerNorm in place, 8 lanes per row
//   head       MU = hb + hW y on virtual waves 0 and 1
//   rows       lane r < 32 of wave 0 forms row r's ratio and KL term (ma_ls_row.h, shared with spo_ma_trpo_linesearch_sums) and
//              adds the four row terms to its fp64 sums; rows past the batch add nothing.  No barrier follows: the other waves
//              start the next chunk, whose first write to MU is four barriers away.
// After the last chunk wave 0 adds its 32 lanes' sums (xor 16, 8, 4, 2, 1) and writes ONE quadruple.  No atomics: repeats are
// bit-identical.
#include "common.h"
#include "rows_frag.h"
#include "ma_layout.h"
#include "ma_ls_row.h"

namespace {
using namespace spo;
using namespace spo::rows;

constexpr int MAXB = 2;                    // blocks
constexpr float LN_EPS = 1e-5f;            // nn.LayerNorm's default, as ma_net.hip
static_assert(MAX_GRID * MA_LS_NS <= SPO_MA_LS_WS_DOUBLES, "ma_ls_eval: one quadruple per workgroup in partial_ws");
static_assert(MAXA == SPO_MAX_ACT, "ma_ls_eval: one head tile");
static_assert(MAXW <= 128, "ma_ls_eval: the fold's dot product takes columns lane and lane + 64");

struct LsArgs {
  int D, H, O;
  int64_t B;
  int vec4;                                // obs rows are 16-byte aligned: float4 loads
  float xc, yc;
  const float* theta; const float* obs; const float* act; const float* old_logp; const float* adv; const float* cost_adv;
  const float* factor; const float* mu_old; const float* std_old;
  int w[MAXB + 1], b[MAXB + 1], g[MAXB], be[MAXB], logstd;      // offsets in theta; index NB: the head
  float* ratio_out; double* partial;
};

constexpr int LDS_FLOATS = 3 * IMG + ROWS * LDO + MAXW + 3 * MAXA;

__device__ __forceinline__ float elu(float z) { return z > 0.f ? z : expm1f(z); }      // nn.ELU(alpha=1)

// mm_rows (rows_frag.h) on W diag(gam): the fold of the input LayerNorm's weight, formed on the fragments
__device__ __forceinline__ void mm_rows_scaled(const float* __restrict__ Wg, const float* __restrict__ gam, int out, int in, const float* IN,
                                               const Unit u, int j, int q, f4 (&acc)[2]) {
  const int nk = (in + 15) >> 4;
  f4 af[MAXT];
#pragma unroll
  for (int nt = 0; nt < MAXT; ++nt)
    if (nt < nk) af[nt] = ld_row4(Wg, in, 16 * u.t + j, out, 16 * nt + 4 * q, in) * bias4(gam, 16 * nt + 4 * q, in);
#pragma unroll
  for (int nt = 0; nt < MAXT; ++nt)
    if (nt < nk) {
      f4 b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
        if (i < u.nr) b[i] = *reinterpret_cast<const f4*>(IN + (16 * (u.r0 + i) + j) * LDI + 16 * nt + 4 * q);
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int i = 0; i < 2; ++i)
          if (i < u.nr) acc[i] = mfma4(af[nt][r], b[i][r], acc[i]);
    }
}

template <int NB>
__global__ __launch_bounds__(NTHR, 1) void ma_ls_eval_kernel(LsArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  float* const X = lds;
  float* const P = lds + IMG;
  float* const MU = lds + 3 * IMG;
  float* const BF = MU + ROWS * LDO;
  float* const DC = BF + MAXW;
  const int D = a.D, H = a.H, Od = a.O;
  const int nth = (H + 15) >> 4, Hp = 16 * nth;
  const float inv_d = 1.f / (float)D, inv_h = 1.f / (float)H;

  // ---- prologue: b'_0[n] = b_0[n] + W_0[n] . beta, one wave per output row, lanes and order of fn_fold_kernel
  {
    const float* W0 = a.theta + a.w[0];
    const float* bet = a.theta + D;
    // sixteen rows' loads in flight at a time (in_dim <= 128: columns lane and lane + 64, in that order)
    const bool c0ok = lane < D, c1ok = lane + 64 < D;
    const float bet0 = bet[c0ok ? lane : 0], bet1 = bet[c1ok ? lane + 64 : 0];
    for (int n0 = wave; n0 < H; n0 += 16 * (NTHR / 64)) {
      float w0[16], w1[16], b0[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int n = n0 + u * (NTHR / 64) < H ? n0 + u * (NTHR / 64) : H - 1;      // addresses clamped, never predicated
        w0[u] = W0[n * D + (c0ok ? lane : 0)]; w1[u] = W0[n * D + (c1ok ? lane + 64 : 0)]; b0[u] = a.theta[a.b[0] + n];
      }
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        float dot = c0ok ? fmaf(w0[u], bet0, 0.f) : 0.f;
        if (c1ok) dot = fmaf(w1[u], bet1, dot);
        dot = wave_sum_all(dot);
        if (lane == 0 && n0 + u * (NTHR / 64) < H) BF[n0 + u * (NTHR / 64)] = b0[u] + dot;
      }
    }
    if (tid < Od) ma_ls_dim_consts(a.theta[a.logstd + tid], a.std_old[tid], a.xc, a.yc, DC[tid], DC[MAXA + tid], DC[2 * MAXA + tid]);
  }
  double acc[MA_LS_NS] = {0, 0, 0, 0};

  const int64_t nchunks = (a.B + ROWS - 1) / ROWS;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    // the lane coordinates are derived from an opaque copy of the thread index once per chunk: every weight fragment's address
    // depends on them, and as loop invariants of the chunk loop the fragments themselves would be hoisted out of it and spilled
    int ot = tid;
    asm volatile("" : "+v"(ot));
    const int j = ot & 15, q = (ot >> 4) & 3, rrow = ot >> 3, s8 = ot & 7;
    const int64_t row0 = c * ROWS;
    // ---- N: the input LayerNorm, raw row -> registers -> X (pre-affine: gamma / beta are folded into block 0)
    {
      const int64_t grow = row0 + rrow;
      const bool rok = grow < a.B;
      const float* src = a.obs + (rok ? grow : 0) * D;      // addresses clamped, never predicated
      f4 v[4];
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c0 = 32 * i + 4 * s8;
        if (a.vec4) {
          const f4 t = *reinterpret_cast<const f4*>(src + (c0 < D ? c0 : 0));
#pragma unroll
          for (int e = 0; e < 4; ++e) v[i][e] = (rok && c0 < D) ? t[e] : 0.f;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float t = src[c0 + e < D ? c0 + e : 0];
            v[i][e] = (rok && c0 + e < D) ? t : 0.f;
          }
        }
        s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
      }
      const float mean = sum8(s) * inv_d;
      float sq = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = 32 * i + 4 * s8 + e < D ? v[i][e] - mean : 0.f;
          v[i][e] = d; sq += d * d;
        }
      const float rstd = 1.f / sqrtf(sum8(sq) * inv_d + LN_EPS);          // biased variance, as nn.LayerNorm
#pragma unroll
      for (int i = 0; i < 4; ++i) *reinterpret_cast<f4*>(X + rrow * LDI + 32 * i + 4 * s8) = v[i] * rstd;
    }
    __syncthreads();

#pragma unroll
    for (int k = 0; k < NB; ++k) {
      const float* IN = k == 0 ? X : P + ((k - 1) & 1) * IMG;
      float* const Z = P + (k & 1) * IMG;
      // ---- T: a = ELU(b + W IN); columns H .. Hp get ELU(0) = 0
#pragma unroll
      for (int s = 0; s < VW; ++s) {
        const Unit u = unit_of(wave + 4 * s, nth);
        if (u.on) {
          const int f0 = 16 * u.t + 4 * q;
          f4 t[2];
          t[0] = t[1] = k == 0 ? bias4(BF, f0, H) : bias4(a.theta + a.b[k], f0, H);
          __builtin_amdgcn_sched_barrier(0);
          if (k == 0) mm_rows_scaled(a.theta + a.w[0], a.theta, H, D, IN, u, j, q, t);
          else mm_rows(a.theta + a.w[k], H, H, IN, u, j, q, t);
#pragma unroll
          for (int i = 0; i < 2; ++i)
            if (i < u.nr) {
#pragma unroll
              for (int r = 0; r < 4; ++r) t[i][r] = elu(t[i][r]);
              *reinterpret_cast<f4*>(Z + (16 * (u.r0 + i) + j) * LDI + f0) = t[i];
            }
        }
        __builtin_amdgcn_sched_barrier(0);            // one virtual wave's fragments at a time
      }
      __syncthreads();
      // ---- L: y = (a - mean) rstd g + be in place; a lane reads and writes its own columns only
      {
        float* const zr = Z + rrow * LDI;
        f4 v[4];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int c0 = 32 * i + 4 * s8;
          v[i] = f4{0.f, 0.f, 0.f, 0.f};
          if (c0 < Hp) v[i] = *reinterpret_cast<const f4*>(zr + c0);
          s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
        }
        const float mean = sum8(s) * inv_h;
        float sq = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float d = 32 * i + 4 * s8 + e < H ? v[i][e] - mean : 0.f;
            v[i][e] = d; sq += d * d;
          }
        const float rstd = 1.f / sqrtf(sum8(sq) * inv_h + LN_EPS);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int c0 = 32 * i + 4 * s8;
          if (c0 < Hp) {
            const f4 g4 = bias4(a.theta + a.g[k], c0, H), be4 = bias4(a.theta + a.be[k], c0, H);
            f4 y;
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = v[i][e] * rstd * g4[e] + be4[e];
            *reinterpret_cast<f4*>(zr + c0) = y;
          }
        }
      }
      __syncthreads();
    }

    // ---- head: mu = hb + hW y
    {
      const Unit u = unit_of(wave, 1);
      if (u.on) {
        f4 t[2];
        t[0] = t[1] = bias4(a.theta + a.b[NB], 4 * q, Od);
        mm_rows(a.theta + a.w[NB], Od, H, P + ((NB - 1) & 1) * IMG, u, j, q, t);
        *reinterpret_cast<f4*>(MU + (16 * u.r0 + j) * LDO + 4 * q) = t[0];
      }
    }
    __syncthreads();

    // ---- rows
    if (tid < ROWS && row0 + tid < a.B) {
      const int64_t r = row0 + tid;
      // the row's inputs in flight together (addresses clamped to the row), then the dimensions in order
      float av[MAXA], ol[MAXA], mo[MAXA];
#pragma unroll
      for (int d = 0; d < MAXA; ++d) {
        const int64_t i = r * Od + (d < Od ? d : 0);
        av[d] = a.act[i]; ol[d] = a.old_logp[i]; mo[d] = a.mu_old[i];
      }
      const float fr = a.factor[r], ar = a.adv[r], cr = a.cost_adv[r];
      float ratio = 1.f, kl = 0.f;
#pragma unroll
      for (int d = 0; d < MAXA; ++d)
        if (d < Od) ma_ls_dim_term(MU[tid * LDO + d], av[d], ol[d], mo[d], DC[d], DC[MAXA + d], DC[2 * MAXA + d], ratio, kl);
      ma_ls_row_add(ratio, kl, fr, ar, cr, acc);
      if (a.ratio_out) a.ratio_out[r] = ratio;
    }
  }

  // ---- this workgroup's quadruple: lanes 0 .. 31 of wave 0 hold the sums (the other lanes of the wave: zeros)
  if (wave == 0) {
#pragma unroll
    for (int k = 0; k < MA_LS_NS; ++k) {
      double v = acc[k];
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if (lane == 0) a.partial[(int64_t)blockIdx.x * MA_LS_NS + k] = v;
    }
  }
}

// sums_out[k] = sum over the workgroups' quadruples: wave k, lane l adds quadruples l, l + 64, ... in order, then the lanes
__global__ __launch_bounds__(64 * MA_LS_NS) void ma_ls_eval_reduce_kernel(const double* __restrict__ partial, int nparts,
                                                                           double* __restrict__ sums_out) {
  const int lane = threadIdx.x & 63, k = threadIdx.x >> 6;
  double v = 0.0;
  for (int b = lane; b < nparts; b += 64) v += partial[(int64_t)b * MA_LS_NS + k];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if (lane == 0) sums_out[k] = v;
}

// the envelope; 0, or -1 / -2 with the dimension named
int ls_lay(const spo_ma_net* net, Lay* L) {
  if (int rc = lay_of(net, L)) return rc;
  if (!L->actor) return fail(-2, "ma_ls_eval: is_actor 0, the kernel takes an actor (the critics have no line search)");
  if (L->H > MAXW) return fail(-2, "ma_ls_eval: hidden %d outside [1,%d]", L->H, MAXW);
  if (L->D > MAXW) return fail(-2, "ma_ls_eval: in_dim %d outside [1,%d]", L->D, MAXW);
  if (L->O > MAXA) return fail(-2, "ma_ls_eval: out_dim %d outside [1,%d]", L->O, MAXA);
  if (L->NB > MAXB) return fail(-2, "ma_ls_eval: n_blocks %d outside [1,%d]", L->NB, MAXB);
  return 0;
}

template <int NB>
int launch(const LsArgs& a, int blocks, hipStream_t st) {
  constexpr size_t bytes = LDS_FLOATS * sizeof(float);
  static_assert(bytes <= 64 * 1024, "ma_ls_eval: the chunk's images fit the default LDS limit");
  static bool attr_done[SPO_MAX_DEVICES] = {};
  return launch_dyn_lds(&ma_ls_eval_kernel<NB>, attr_done, "ma_ls_eval", dim3(blocks), dim3(NTHR), bytes, st, a);
}

}  // namespace

extern "C" int spo_ma_ls_eval_supported(const spo_ma_net* net) {
  Lay L;
  return (net && ls_lay(net, &L) == 0) ? 1 : 0;
}

extern "C" int spo_ma_ls_eval(const float* theta, const spo_ma_net* net, const float* obs, float std_x_coef, float std_y_coef,
                              const float* act, const float* old_logp, const float* adv, const float* cost_adv, const float* factor,
                              const float* mu_old, const float* std_old, int64_t rows, double* sums4_out, float* ratio_out_or_null,
                              double* partial_ws, void* stream) {
  Lay L;
  if (int rc = ls_lay(net, &L)) return rc;
  SPO_REQUIRE(theta && obs && act && old_logp && adv && cost_adv && factor && mu_old && std_old && sums4_out && partial_ws,
              "ma_ls_eval: bad args (null pointer)");
  SPO_REQUIRE(rows >= 1, "ma_ls_eval: bad args (rows %lld)", (long long)rows);
  hipStream_t st = (hipStream_t)stream;
  LsArgs a{};
  a.D = L.D; a.H = L.H; a.O = L.O; a.B = rows;
  a.vec4 = (L.D % 4 == 0) && reinterpret_cast<uintptr_t>(obs) % 16 == 0;
  a.xc = std_x_coef; a.yc = std_y_coef;
  a.theta = theta; a.obs = obs; a.act = act; a.old_logp = old_logp; a.adv = adv; a.cost_adv = cost_adv; a.factor = factor;
  a.mu_old = mu_old; a.std_old = std_old;
  for (int k = 0; k < L.NB; ++k) { a.w[k] = (int)L.W(k); a.b[k] = (int)L.b(k); a.g[k] = (int)L.g(k); a.be[k] = (int)L.be(k); }
  a.w[L.NB] = (int)L.hW(); a.b[L.NB] = (int)L.hb(); a.logstd = (int)L.logstd();
  a.ratio_out = ratio_out_or_null; a.partial = partial_ws;
  const int64_t nchunks = (rows + ROWS - 1) / ROWS;
  const int blocks = (int)(nchunks < MAX_GRID ? nchunks : MAX_GRID);
  if (int rc = L.NB == 1 ? launch<1>(a, blocks, st) : launch<2>(a, blocks, st)) return rc;
  hipLaunchKernelGGL(ma_ls_eval_reduce_kernel, dim3(1), dim3(64 * MA_LS_NS), 0, st, partial_ws, blocks, sums4_out);
  SPO_LAUNCH_CHECK("spo_ma_ls_eval");
  return 0;
}
