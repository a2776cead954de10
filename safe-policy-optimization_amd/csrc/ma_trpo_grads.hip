// MACPO's two surrogate gradients in one fused pass for the multi-agent actor, hidden width <= 128, gfx950 (spo_ma_trpo_grads).
//
// Reference: safepo/multi_agent/macpo.py:238-249 differentiates -mean(factor * ratio * adv) and the same with cost_adv.  The
// launch-per-layer path runs spo_ma_actor_loss + spo_ma_backward once per gradient.  With the clip off and no entropy term the
// cotangent of the head output is  adv[row] * u[row, :]  resp.  cost_adv[row] * u[row, :]  with ONE
//   u = -(factor * ratio / rows_global) * d logp / d mean,
// and backpropagation is linear in it: the per-row delta chain (W^T products, ELU', LayerNorm backward) is walked once on u, and
// only the weight-gradient sums are formed twice,  dW_r = sum_rows adv * delta_u (x) a,  dW_c = sum_rows cost_adv * delta_u (x) a.
// Nothing is ever divided by an advantage: a row with adv == 0 adds exactly 0 to the reward gradient.
// Four launches: ma_trpo_grads_kernel, the fixed-order reduction, and the input LayerNorm's unfold (fn_unfold_grad_kernel) once per
// gradient.  Envelope (spo_ma_trpo_grads_supported): the one of spo_ma_fvp -- an actor, in_dim 1..128, hidden 1..128, out_dim 1..16,
// 1 or 2 blocks.
//
// Grid, chunk loop, masked tail and the backward sub-phases are those of ma_fvp_kernel (ma_fvp.hip): at most 256 workgroups of 256
// threads, workgroup b walks the 32-row chunks b, b + gridDim.x, ...; the forward activations are LOADED from the workspace
// spo_ma_forward left.  LDS row images [32][132]: X, A[k], Y[k], TB[k] (dy_k, then dz_k in place), O [32][20] (u), ST[k] / RM (row
// statistics / the two row means of a LayerNorm backward), SC [2][32] (the chunk's adv and cost_adv, zero past the batch) and DC
// [2][16] (std and d std / d log_std per action dimension).  NB = 2: 7 x 16 896 + 2 560 + 768 + 256 + 128 = 121 984 B; NB = 1: 71 040 B.
//
// Sub-phases of one chunk, one barrier after each:
//   1          the images <- ws;  H: 8 lanes per row form the row's ratio (every lane, dimensions in order, as ma_actor_loss_kernel),
//              lane s8 the dimensions s8 and s8 + 8 of u and of the log_std row term; lane 0 of the row the two row losses and SC
//   backward, layer l = NB .. 0 (ma_fvp.hip's W / LR / LC):
//              W   dW_l[g] += (sc_g dz_l)^T IN_l: the dz fragment is scaled by the row's adv resp. cost_adv as it is loaded and
//                  feeds one MFMA per gradient; dy_{l-1} = dz_l W_l once, on the unscaled image
//              LR  the two row means of the LayerNorm backward, once
//              LC  thread = (feature, half of the rows): d(ln weight), d(ln bias), d(linear bias) per gradient, dz in place once
// NG = 2: both gradients' accumulators stay resident across the chunks (NB = 1: 160 per lane; NB = 2: 288).  NG = 1 is the split
// form: gridDim.y = 2, blockIdx.y names the gradient, every workgroup walks the delta chain itself.  Which instantiation ships is
// decided by the compiler's report (profiles/ma_trpo_grads/resource_usage.txt): no form with a scratch frame is launched.
// After the last chunk a workgroup writes one partial vector per gradient, every element exactly once (the input LayerNorm's and
// log_std's slots as zeros), and one fp64 record per gradient {row-loss sum, log_std row sums [16]}.  No atomics: repeats are
// bit-identical.
#include "common.h"
#include "rows_frag.h"
#include "ma_layout.h"
#include "ma_ls_row.h"

namespace {
using namespace spo;
using namespace spo::rows;

constexpr int MAXB = 2;                    // blocks
constexpr int REC = 1 + MAXA;              // doubles per workgroup and gradient: the row-loss sum, then the log_std row sums
static_assert(MAXA == SPO_MAX_ACT && MAXA == 16, "ma_trpo_grads: a row's eight lanes take two action dimensions each");

struct GradArgs {
  int D, H, O;
  int64_t B;
  float inv_rows_global, xc, yc;
  int vec4;                                // ws is 16-byte aligned: the float4 loads of the images
  const float* theta; const float* mean; const float* act; const float* old_logp; const float* adv; const float* cost_adv;
  const float* factor;
  const float* xhat; const float* a[MAXB]; const float* st[MAXB]; const float* y[MAXB];
  int w[MAXB + 1], b[MAXB + 1], g[MAXB], be[MAXB], logstd;      // offsets in theta; index NB: the head
  int P;
  float* partial; double* rec;
};

template <int NB>
constexpr int lds_floats() { return (1 + 3 * NB) * IMG + ROWS * LDO + (NB + 1) * ROWS * 2 + 2 * ROWS + 2 * MAXA; }

template <int NB, int NG>
__global__ __launch_bounds__(NTHR, 1) void ma_trpo_grads_kernel(GradArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  float* const X = lds;
  float* const A = lds + IMG;
  float* const Y = lds + (1 + NB) * IMG;
  float* const TB = lds + (1 + 2 * NB) * IMG;
  float* const O = lds + (1 + 3 * NB) * IMG;
  float* const ST = O + ROWS * LDO;
  float* const RM = ST + NB * ROWS * 2;
  float* const SC = RM + ROWS * 2;
  float* const DC = SC + 2 * ROWS;
  const int D = a.D, H = a.H, Od = a.O;
  const int nth = (H + 15) >> 4, Hp = 16 * nth;
  const float inv_h = 1.f / (float)H;
  const int chalf = wave >> 1;
  // the advantage of gradient g of this workgroup: both (NG = 2), or the one blockIdx.y names (NG = 1)
  const int g0 = NG == 2 ? 0 : (int)blockIdx.y;
  const float* const scp[2] = {g0 ? a.cost_adv : a.adv, a.cost_adv};

  // std = yc * sigmoid(log_std / xc) and d std / d log_std per action dimension, as ma_actor_loss_kernel (ma_net.hip)
  if (tid < MAXA) {
    const float s = 1.f / (1.f + expf(-a.theta[a.logstd + (tid < Od ? tid : 0)] / a.xc));
    DC[tid] = s * a.yc;
    DC[MAXA + tid] = a.yc * s * (1.f - s) / a.xc;
  }
  __syncthreads();

  f4 accW[NG][VW][NB][MAXT];
  f4 accO[NG][MAXT / 2];                   // the head is one band: virtual waves 0 and 1, every other tile
  float dhb[NG];
  float cg[NG][NB], cb[NG][NB], cz[NG][NB];      // this thread's feature: d(ln weight), d(ln bias), d(linear bias) of block k
  double loss[NG], dls[NG][2];             // lane s8 of a row: action dimensions s8 and s8 + 8; the row loss on lane 0
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    dhb[g] = 0.f; loss[g] = 0.0; dls[g][0] = dls[g][1] = 0.0;
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      cg[g][k] = cb[g][k] = cz[g][k] = 0.f;
#pragma unroll
      for (int s = 0; s < VW; ++s)
#pragma unroll
        for (int i = 0; i < MAXT; ++i) accW[g][s][k][i] = f4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int i = 0; i < MAXT / 2; ++i) accO[g][i] = f4{0.f, 0.f, 0.f, 0.f};
  }

  const int64_t nchunks = (a.B + ROWS - 1) / ROWS;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    // the lane coordinates are derived from an opaque copy of the thread index once per chunk (ma_fvp.hip): as loop invariants of
    // the chunk loop the fragment addresses and masks would take more registers than the accumulators
    int ot = tid;
    asm volatile("" : "+v"(ot));
    const int j = ot & 15, q = (ot >> 4) & 3, rrow = ot >> 3, s8 = ot & 7, ccol = ot & (MAXW - 1);
    const int64_t row0 = c * ROWS;
    // ---- 1: the saved activations
    load_image(X, a.xhat, D, row0, a.B, a.vec4 && (D & 3) == 0, tid);
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      load_image(A + k * IMG, a.a[k], H, row0, a.B, a.vec4 && (H & 3) == 0, tid);
      load_image(Y + k * IMG, a.y[k], H, row0, a.B, a.vec4 && (H & 3) == 0, tid);
      if (tid < 2 * ROWS) {
        const int64_t grow = row0 + (tid >> 1);
        ST[k * ROWS * 2 + tid] = grow < a.B ? a.st[k][grow * 2 + (tid & 1)] : 0.f;      // rstd = 0: a row past the batch stays finite
      }
    }
    // ---- H: the head's row terms.  A row past the batch reads row 0 (addresses clamped) and gets u = 0 and both advantages 0.
    {
      const int64_t grow = row0 + rrow;
      const bool rok = grow < a.B;
      const int64_t rr = rok ? grow : 0, rb = rr * Od;
      float ratio = 1.f, dif[2] = {0.f, 0.f};
#pragma unroll
      for (int d = 0; d < MAXA; ++d)
        if (d < Od) {
          float df;
          const float lp = ma_logp_dim(a.mean[rb + d], a.act[rb + d], DC[d], df);
          ratio *= expf(lp - a.old_logp[rb + d]);              // torch.exp per dimension, then torch.prod
          if (d == s8) dif[0] = df;
          if (d == s8 + 8) dif[1] = df;
        }
      const float f = a.factor[rr];
      const float dlp = rok ? -(f * a.inv_rows_global) * ratio : 0.f;      // d(loss) / d logp of every dimension, per unit advantage
      float sc[NG];
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const float t = scp[g][rr];
        sc[g] = rok ? t : 0.f;
        if (s8 == 0) loss[g] += (double)(f * (ratio * sc[g]) * a.inv_rows_global);
      }
      if (s8 < 2) SC[s8 * ROWS + rrow] = s8 < NG ? sc[s8 < NG ? s8 : 0] : 0.f;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int d = s8 + 8 * e;
        float u = 0.f;
        if (d < Od) {
          const float sd = DC[d], iv = 1.f / (sd * sd);
          u = dlp * dif[e] * iv;
          // d logp / d sigma = dif^2 / sigma^3 - 1 / sigma
          const float t = dlp * (dif[e] * dif[e] * iv / sd - 1.f / sd) * DC[MAXA + d];
#pragma unroll
          for (int g = 0; g < NG; ++g) dls[g][e] += (double)(sc[g] * t);
        }
        O[rrow * LDO + d] = u;
      }
    }
    __syncthreads();

    // ---- backward
#pragma unroll
    for (int l = NB; l >= 0; --l) {
      const int in = l == 0 ? D : H, out = l == NB ? Od : H;
      const int ntm = (out + 15) >> 4, ntk = (in + 15) >> 4;
      const float* DZ = l == NB ? O : TB + (l < NB ? l : 0) * IMG;
      const int ldz = l == NB ? LDO : LDI;
      const float* IN = l == 0 ? X : Y + (l - 1) * IMG;
      const bool wide = ntm > 4;
      // W: the weight gradients on the band owners: band mt of 16 output features, tiles kt = k0 + i * ks of 16 input features
#pragma unroll
      for (int s = 0; s < VW; ++s) {
        const int vw = wave + 4 * s;
        const int mt = wide ? vw : vw >> 1, k0 = wide ? 0 : vw & 1, ks = wide ? 1 : 2;
        if (mt < ntm) {
#pragma unroll
          for (int rt = 0; rt < 2; ++rt) {
            const int r0 = 16 * rt + 4 * q;
            float az[NG][4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float z = DZ[(r0 + r) * ldz + 16 * mt + j];
#pragma unroll
              for (int g = 0; g < NG; ++g) az[g][r] = z * SC[g * ROWS + r0 + r];
            }
            if (l == NB && s == 0) {
#pragma unroll
              for (int g = 0; g < NG; ++g) dhb[g] += (az[g][0] + az[g][1]) + (az[g][2] + az[g][3]);
            }
            float bh[MAXT][4];
#pragma unroll
            for (int i = 0; i < MAXT; ++i)
              if (k0 + i * ks < ntk) {
#pragma unroll
                for (int r = 0; r < 4; ++r) bh[i][r] = IN[(r0 + r) * LDI + 16 * (k0 + i * ks) + j];
              }
#pragma unroll
            for (int g = 0; g < NG; ++g)
#pragma unroll
              for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int i = 0; i < MAXT; ++i)
                  if (k0 + i * ks < ntk) {
                    if (l < NB) accW[g][s][l < NB ? l : 0][i] = mfma4(az[g][r], bh[i][r], accW[g][s][l < NB ? l : 0][i]);
                    else if (s == 0 && i < MAXT / 2) accO[g][i] = mfma4(az[g][r], bh[i][r], accO[g][i]);
                  }
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      __builtin_amdgcn_sched_barrier(0);          // the dy fragments stay out of the dW products' register budget
      if (l > 0) {
        float* const DY = TB + (l - 1) * IMG;
#pragma unroll
        for (int s = 0; s < VW; ++s) {
          const Unit u = unit_of(wave + 4 * s, ntk);
          if (u.on) {
            f4 acc[2] = {f4{0.f, 0.f, 0.f, 0.f}, f4{0.f, 0.f, 0.f, 0.f}};
            mm_cols(a.theta + a.w[l], out, in, DZ, ldz, u, j, q, acc);
#pragma unroll
            for (int i = 0; i < 2; ++i)
              if (i < u.nr) *reinterpret_cast<f4*>(DY + (16 * (u.r0 + i) + j) * LDI + 16 * u.t + 4 * q) = acc[i];
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      __syncthreads();
      if (l > 0) {
        const int kk = l - 1;
        float* const DY = TB + kk * IMG;
        const float* Ak = A + kk * IMG;
        // LR: m1 = mean(g dy), m2 = mean(g dy xhat)
        {
          const float mean = ST[(kk * ROWS + rrow) * 2], rstd = ST[(kk * ROWS + rrow) * 2 + 1];
          float s1 = 0.f, s2 = 0.f;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int c0 = 32 * i + 4 * s8;
            if (c0 < Hp) {
              const f4 dy = *reinterpret_cast<const f4*>(DY + rrow * LDI + c0), av = *reinterpret_cast<const f4*>(Ak + rrow * LDI + c0);
              const f4 g4 = bias4(a.theta + a.g[kk], c0, H);
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const float dxh = dy[e] * g4[e];
                s1 += dxh; s2 += dxh * ((av[e] - mean) * rstd);
              }
            }
          }
          s1 = sum8(s1); s2 = sum8(s2);
          if (s8 == 0) { RM[rrow * 2] = s1 * inv_h; RM[rrow * 2 + 1] = s2 * inv_h; }
        }
        __syncthreads();
        // LC
        if (ccol < H) {
          const float gc = a.theta[a.g[kk] + ccol];
#pragma unroll
          for (int r = 0; r < ROWS / 2; ++r) {
            const int row = chalf * (ROWS / 2) + r;
            const float mean = ST[(kk * ROWS + row) * 2], rstd = ST[(kk * ROWS + row) * 2 + 1];
            const float m1 = RM[row * 2], m2 = RM[row * 2 + 1];
            const float dy = DY[row * LDI + ccol], av = Ak[row * LDI + ccol];
            const float xh = (av - mean) * rstd;
            const float dz = rstd * (dy * gc - m1 - xh * m2) * elu_grad(av);
#pragma unroll
            for (int g = 0; g < NG; ++g) {
              const float sg = SC[g * ROWS + row];
              cg[g][kk] += sg * (dy * xh); cb[g][kk] += sg * dy; cz[g][kk] += sg * dz;
            }
            DY[row * LDI + ccol] = dz;
          }
        }
        __syncthreads();
      }
    }
  }

  // ---- this workgroup's partial vectors: every element written exactly once
  const int j = tid & 15, q = (tid >> 4) & 3, ccol0 = tid & (MAXW - 1), lane = tid & 63;
  float* const red = lds;
  double* const rd = reinterpret_cast<double*>(lds + IMG);      // [4 waves][NG][REC]
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    float* out = a.partial + ((int64_t)blockIdx.x * 2 + g0 + g) * a.P;
#pragma unroll
    for (int l = 0; l <= NB; ++l) {
      const int in = l == 0 ? D : H, outw = l == NB ? Od : H;
      const int ntm = (outw + 15) >> 4, ntk = (in + 15) >> 4;
      const bool wide = ntm > 4;
#pragma unroll
      for (int v = 0; v < VW; ++v) {
        const int vw = wave + 4 * v;
        const int mt = wide ? vw : vw >> 1, k0 = wide ? 0 : vw & 1, ks = wide ? 1 : 2;
        if (mt < ntm) {
#pragma unroll
          for (int i = 0; i < MAXT; ++i) {
            const int k = 16 * (k0 + i * ks) + j;
            if (k0 + i * ks < ntk && k < in) {
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int m = 16 * mt + 4 * q + r;
                if (m < outw) out[a.w[l] + m * in + k] = l < NB ? accW[g][v][l < NB ? l : 0][i][r] : accO[g][v == 0 && i < MAXT / 2 ? i : 0][r];
              }
            }
          }
        }
      }
    }
    {
      float s = dhb[g];                             // waves 0 and 1 both hold the head's band; wave 0 writes it
      s += __shfl_xor(s, 16);
      s += __shfl_xor(s, 32);
      if (wave == 0 && q == 0 && j < Od) out[a.b[NB] + j] = s;
    }
    for (int i = tid; i < 2 * D; i += NTHR) out[i] = 0.f;            // the input LayerNorm: filled by the unfold
    if (tid < Od) out[a.logstd + tid] = 0.f;                         // log_std: the reduction writes it from the fp64 records
    // the two halves' feature sums, half 0 first
    if (chalf == 1) {
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        red[((g * NB + k) * 3) * MAXW + ccol0] = cg[g][k];
        red[((g * NB + k) * 3 + 1) * MAXW + ccol0] = cb[g][k];
        red[((g * NB + k) * 3 + 2) * MAXW + ccol0] = cz[g][k];
      }
    }
    // the fp64 row sums: the rows of a wave (lanes s8 + 8 r), then the waves in order
    double v0 = loss[g], v1 = dls[g][0], v2 = dls[g][1];
#pragma unroll
    for (int o = 8; o < 64; o <<= 1) { v0 += __shfl_xor(v0, o, 64); v1 += __shfl_xor(v1, o, 64); v2 += __shfl_xor(v2, o, 64); }
    if (lane < 8) {
      double* w = rd + (wave * NG + g) * REC;
      if (lane == 0) w[0] = v0;
      w[1 + lane] = v1; w[1 + 8 + lane] = v2;
    }
  }
  __syncthreads();
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    float* out = a.partial + ((int64_t)blockIdx.x * 2 + g0 + g) * a.P;
    if (chalf == 0 && ccol0 < H) {
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        out[a.g[k] + ccol0] = cg[g][k] + red[((g * NB + k) * 3) * MAXW + ccol0];
        out[a.be[k] + ccol0] = cb[g][k] + red[((g * NB + k) * 3 + 1) * MAXW + ccol0];
        out[a.b[k] + ccol0] = cz[g][k] + red[((g * NB + k) * 3 + 2) * MAXW + ccol0];
      }
    }
    if (tid < REC)
      a.rec[((int64_t)blockIdx.x * 2 + g0 + g) * REC + tid] =
          (rd[(0 * NG + g) * REC + tid] + rd[(1 * NG + g) * REC + tid]) + (rd[(2 * NG + g) * REC + tid] + rd[(3 * NG + g) * REC + tid]);
  }
}

// blockIdx.y = gradient g.  Blocks 0 .. gridDim.x - 2: grad_g[i] = sum_k partial[k][g][i] in the order of k, sixteen loads in flight at
// a time.  The last block: the fp64 records in the order of k -> losses[g] = -(row-loss sum), grad_g's log_std slot.
__global__ __launch_bounds__(64) void ma_trpo_grads_reduce_kernel(const float* __restrict__ partial, const double* __restrict__ rec,
                                                                  int nparts, int P, int logstd, int Od, float* __restrict__ grad_r,
                                                                  float* __restrict__ grad_c, float* __restrict__ losses) {
  const int g = blockIdx.y;
  float* const grad = g ? grad_c : grad_r;
  if (blockIdx.x == gridDim.x - 1) {
    const int t = threadIdx.x;
    if (t > Od) return;
    double s = 0.0;
    int k = 0;
    for (; k + 16 <= nparts; k += 16) {
      double v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = rec[((int64_t)(k + u) * 2 + g) * REC + t];
#pragma unroll
      for (int u = 0; u < 16; ++u) s += v[u];
    }
    for (; k < nparts; ++k) s += rec[((int64_t)k * 2 + g) * REC + t];
    if (t == 0) losses[g] = (float)(-s);
    else grad[logstd + t - 1] = (float)s;
    return;
  }
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P || (i >= logstd && i < logstd + Od)) return;
  float acc = 0.f;
  int k = 0;
  for (; k + 16 <= nparts; k += 16) {
    float v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = partial[((int64_t)(k + u) * 2 + g) * P + i];
#pragma unroll
    for (int u = 0; u < 16; ++u) acc += v[u];
  }
  for (; k < nparts; ++k) acc += partial[((int64_t)k * 2 + g) * P + i];
  grad[i] = acc;
}

// the envelope; 0, or -1 / -2 with the dimension named
int grads_lay(const spo_ma_net* net, Lay* L) {
  if (int rc = lay_of(net, L)) return rc;
  if (!L->actor) return fail(-2, "ma_trpo_grads: is_actor 0, the kernel takes an actor (the critics have no surrogate)");
  if (L->H > MAXW) return fail(-2, "ma_trpo_grads: hidden %d outside [1,%d]", L->H, MAXW);
  if (L->D > MAXW) return fail(-2, "ma_trpo_grads: in_dim %d outside [1,%d]", L->D, MAXW);
  if (L->O > MAXA) return fail(-2, "ma_trpo_grads: out_dim %d outside [1,%d]", L->O, MAXA);
  if (L->NB > MAXB) return fail(-2, "ma_trpo_grads: n_blocks %d outside [1,%d]", L->NB, MAXB);
  return 0;
}

int num_partials(int64_t rows) {
  const int64_t n = (rows + ROWS - 1) / ROWS;
  return (int)(n < 1 ? 1 : n < MAX_GRID ? n : MAX_GRID);
}

template <int NB, int NG>
int launch(const GradArgs& a, int blocks, hipStream_t st) {
  constexpr size_t bytes = lds_floats<NB>() * sizeof(float);
  static_assert(bytes <= 160 * 1024, "ma_trpo_grads: the chunk's images do not fit one workgroup's LDS");
  static_assert(2 * 3 * MAXB * MAXW <= IMG && 4 * 2 * REC * 2 <= IMG, "ma_trpo_grads: the final sums reuse the first two images");
  static bool attr_done[SPO_MAX_DEVICES] = {};
  return launch_dyn_lds(&ma_trpo_grads_kernel<NB, NG>, attr_done, "ma_trpo_grads", dim3(blocks, 2 / NG), dim3(NTHR), bytes, st, a);
}

}  // namespace

extern "C" int spo_ma_trpo_grads_supported(const spo_ma_net* net) {
  Lay L;
  return (net && grads_lay(net, &L) == 0) ? 1 : 0;
}

extern "C" int spo_ma_trpo_grads_num_partials(int64_t rows) { return num_partials(rows); }

// scratch per workgroup: two fp64 records of 1 + 16 doubles (first, so that they are 8-byte aligned), then two partial vectors
extern "C" int64_t spo_ma_trpo_grads_scratch_floats(const spo_ma_net* net, int64_t rows) {
  Lay L;
  if (grads_lay(net, &L) || rows < 1) return -1;
  return (int64_t)num_partials(rows) * 2 * (2 * REC + L.count());
}

extern "C" int spo_ma_trpo_grads(const float* theta, const spo_ma_net* net, const float* ws, const float* mean, const float* act,
                                 const float* old_logp, const float* adv, const float* cost_adv, const float* factor,
                                 float std_x_coef, float std_y_coef, int64_t rows, int64_t rows_global, float* scratch,
                                 float* grad_r, float* grad_c, float* losses2, void* stream) {
  Lay L;
  if (int rc = grads_lay(net, &L)) return rc;
  SPO_REQUIRE(theta && ws && mean && act && old_logp && adv && cost_adv && factor && scratch && grad_r && grad_c && losses2,
              "ma_trpo_grads: bad args (null pointer)");
  SPO_REQUIRE(rows > 0 && rows_global >= rows, "ma_trpo_grads: bad args (rows %lld, rows_global %lld)", (long long)rows,
              (long long)rows_global);
  SPO_REQUIRE(reinterpret_cast<uintptr_t>(scratch) % 8 == 0, "ma_trpo_grads: bad args (scratch is not 8-byte aligned)");
  hipStream_t st = (hipStream_t)stream;
  const int64_t B = rows;
  const int blocks = num_partials(B);
  GradArgs a{};
  a.D = L.D; a.H = L.H; a.O = L.O; a.B = B;
  a.inv_rows_global = 1.f / (float)rows_global; a.xc = std_x_coef; a.yc = std_y_coef;
  a.vec4 = reinterpret_cast<uintptr_t>(ws) % 16 == 0;
  a.theta = theta; a.mean = mean; a.act = act; a.old_logp = old_logp; a.adv = adv; a.cost_adv = cost_adv; a.factor = factor;
  a.xhat = ws + L.ws_xhat();
  for (int k = 0; k < L.NB; ++k) {
    a.a[k] = ws + L.ws_a(B, k); a.st[k] = ws + L.ws_st(B, k); a.y[k] = ws + L.ws_y(B, k);
    a.w[k] = (int)L.W(k); a.b[k] = (int)L.b(k); a.g[k] = (int)L.g(k); a.be[k] = (int)L.be(k);
  }
  a.w[L.NB] = (int)L.hW(); a.b[L.NB] = (int)L.hb(); a.logstd = (int)L.logstd();
  a.P = (int)L.count();
  a.rec = reinterpret_cast<double*>(scratch);
  a.partial = scratch + (int64_t)blocks * 2 * 2 * REC;
  // one block: both gradients resident; two blocks: the split form (both resident needs a scratch frame of 88 B per lane)
  if (int rc = L.NB == 1 ? launch<1, 2>(a, blocks, st) : launch<2, 1>(a, blocks, st)) return rc;
  hipLaunchKernelGGL(ma_trpo_grads_reduce_kernel, dim3((a.P + 63) / 64 + 1, 2), dim3(64), 0, st, a.partial, a.rec, blocks, a.P,
                     a.logstd, L.O, grad_r, grad_c, losses2);
  // grad + W(0) holds dW' = dz_0^T xhat: turn it into dW_0 and read the input LayerNorm's two gradients off it, per gradient
  for (float* grad : {grad_r, grad_c})
    hipLaunchKernelGGL(fn_unfold_grad_kernel, dim3((L.D + 63) / 64), dim3(64), 0, st, theta + L.W(0), theta + L.fn_g(), theta + L.fn_b(),
                       grad + L.W(0), grad + L.b(0), L.H, L.D, grad + L.fn_g(), grad + L.fn_b());
  SPO_LAUNCH_CHECK("spo_ma_trpo_grads");
  return 0;
}
