// CPO full-batch actor kernels for hidden widths other than [64, 64], gfx950 (the spo_cpo_rows_* entry points).
//
// Reference: safepo/single_agent/cpo.py  :356-381 surrogate gradient, :132-157 Fisher-vector product, :473-491 line-search sums.
// Envelope: a tanh MLP actor of two hidden layers, each of width 1..128, obs_dim 1..128, act_dim 1..16
// (spo_cpo_rows_supported; the kernel is written for NL hidden layers, but NL = 3 does not fit the register file without a
// scratch frame and is not instantiated).  cpo.hip keeps the whole [64, 64] network in LDS and mlp_rows.hip writes one partial gradient per
// 16-row group; neither scales to 524 288 rows of a [128, 128, 128] network, so this file has a layout of its own.
//
// Grid: at most 256 workgroups (one per CU) of 256 threads = 4 waves, one per SIMD with 512 registers each; every wave plays two
// of eight "virtual waves" w (= wave and wave + 4) one after the other.  Workgroup b walks the 32-row chunks b, b + gridDim, ...
// Weights are never staged: every wave reads its A fragments (v_mfma_f32_16x16x4_f32, exact fp32) straight from global memory,
// where the 50 k floats of the network are L2-resident; one fragment feeds both 16-row tiles of the chunk.  LDS holds only the
// chunk's activations as ROW images [32][132] (stride 16 n + 4: the row-wise b128 operand reads and the column-wise b32 reads
// of the weight-gradient products both spread over all banks, so no transposed copies are kept):
//
//   X            observations, zero beyond obs_dim                                  32 x 132
//   H[0..NL-1]   tanh outputs of the hidden layers, zero beyond the real width      32 x 132 each
//   TB[0], TB[1] gradient modes only.  Forward of the product: the tangent of hidden layer l in TB[l & 1];
//                backward of both: dZ of hidden layer l in TB[l & 1]                32 x 132 each
//   O            mu (surrogate, line search, mean) or the output tangent (product), then dO in place     32 x 20
//   NL = 2: 5 x 16 896 + 2 560 = 87 040 B;  forward-only modes 53 248 B.
//
// Sub-phases of one chunk, one barrier after each:
//   1        X <- obs rows (rows past the batch: zeros, and their dO is zero)
//   2..      layer l = 0..NL: virtual wave w owns output-feature tile w and both row tiles (widths <= 64 and the output layer: tile w / 2,
//            row tile w & 1).  acc = b + W IN; product mode also t = vb + V IN + W T_in, T_out = (1 - h^2) t: the direction's
//            fragments are read like the weights, the tangent travels with the forward pass.
//   NL + 3   256 threads x 2 = 32 rows x 16 action slots: log-prob, ratio, dO (surrogate) / dO = (J v) / sigma^2 / (M A) (product) /
//            the three line-search sums / the mean written out.
//   NL + 4.. layer l = NL..0: dW_l += dZ_l^T IN_l on the owner waves (below), and dZ_{l-1} = (W_l^T dZ_l) (1 - H_{l-1}^2) with the
//            forward's split over feature tiles of layer l - 1.
// Weight gradients never leave the MFMA accumulators inside the chunk loop: virtual wave w owns the 16-row band w of every dW_l
// (all up to eight 16-column tiles; bands <= 4: band w / 2, every other tile): 2 x 32 accumulator registers per hidden layer and
// wave, 16 for the output layer, 144 at NL = 2.
// After the last chunk the workgroup writes ONE partial vector (every element exactly once); cpo_rows_reduce_kernel adds the
// partials in fixed order.  No atomics: repeats are bit-identical.
// The line-search and the mean mode are the same kernel body (forward only), so the KL at unchanged parameters is exactly 0.
// theta / vec / out: the wide engine's actor layout [log_std | W_0 b_0 | W_1 b_1 | ...], W row-major [out, in].
#include "common.h"
#include "mlp_mfma.h"
#include "rows_frag.h"
#include "../../include/safepo_hip.h"

namespace {
using namespace spo;
using namespace spo::rows;

enum { M_SURR = 0, M_FVP = 1, M_LS = 2, M_MEAN = 3 };

struct RowsNet {
  int n;                                   // Linear layers: hidden + 1
  int dims[SPO_MLP_MAX_LAYERS + 1];
  int w[SPO_MLP_MAX_LAYERS], b[SPO_MLP_MAX_LAYERS];      // offsets in the actor layout (log_std first)
  int Pa;
};

struct RowsArgs {
  RowsNet net;
  const float* theta; const float* vec; const float* obs; const float* act; const float* logp_old;
  const float* adv; const float* adv2; const float* mean_old; const float* log_std_old;
  int64_t M; float sign;
  float* partial; double* partial_loss; double* ls_partials; float* mean_out;
};

template <int NL, int MODE>
constexpr int lds_floats() {
  return ((MODE == M_SURR || MODE == M_FVP) ? 3 + NL : 1 + NL) * IMG + ROWS * LDO;
}

template <int NL, int MODE>
__global__ __launch_bounds__(NTHR, 1) void cpo_rows_kernel(RowsArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr bool GRAD = MODE == M_SURR || MODE == M_FVP;
  constexpr int NLAY = NL + 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j0 = lane & 15, q0 = lane >> 4;
  float* const X = lds;
  float* const H = lds + IMG;
  float* const TB = lds + (1 + NL) * IMG;                       // gradient modes only
  float* const O = lds + (GRAD ? 3 + NL : 1 + NL) * IMG;
  const RowsNet& net = a.net;
  const int D = net.dims[0], A = net.dims[NLAY];

  // the loss sub-phase: thread = (row lrow, action slot ai)
  const int ai = tid & 15;
  const bool on = ai < A;
  const float lsv = on ? a.theta[ai] : 0.f;
  const float sdn = expf(lsv);
  const float ivar = 1.f / (sdn * sdn);
  const float amask = on ? 1.f : 0.f;
  const float inv_m = (float)(1.0 / (double)a.M);
  const float inv_ma = (float)(1.0 / ((double)a.M * (double)A));
  float sdo = 1.f, lsd = 0.f;
  if (MODE == M_SURR) lsd = on ? lsv + LOG_SQRT_2PI : 0.f;
  if (MODE == M_LS) {
    sdo = on ? expf(a.log_std_old[ai]) : 1.f;
    lsd = on ? logf(sdn) + LOG_SQRT_2PI : 0.f;
  }
  float dls = 0.f;
  double lsum = 0.0, s_r = 0.0, s_c = 0.0, s_kl = 0.0;

  // weight-gradient ownership: band mt of 16 output features, tiles kt = k0 + i * ks of 16 input features
  f4 accW[VW][NL][MAXT];
  f4 accO[MAXT / 2];                       // the output layer is one band: virtual waves 0 and 1, every other tile
  float db[VW][NLAY];
  if (GRAD) {
#pragma unroll
    for (int s = 0; s < VW; ++s)
#pragma unroll
      for (int l = 0; l < NLAY; ++l) {
        db[s][l] = 0.f;
#pragma unroll
        for (int i = 0; i < MAXT; ++i)
          if (l < NL) accW[s][l][i] = f4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
    for (int i = 0; i < MAXT / 2; ++i) accO[i] = f4{0.f, 0.f, 0.f, 0.f};
  }

  const int64_t nchunks = (a.M + ROWS - 1) / ROWS;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    // the lane coordinates are made opaque once per chunk: every fragment address and bounds mask below depends on them, and
    // hoisted out of the chunk loop as loop invariants they would take more registers than the accumulators
    int j = j0, q = q0;
    asm volatile("" : "+v"(j), "+v"(q));
    // ---- 1: X
#pragma unroll
    for (int hh = 0; hh < ROWS * 16 / NTHR; ++hh) {
      const int lrow = (tid >> 4) + hh * (NTHR / 16);
      const int64_t grow = c * ROWS + lrow;
      const bool valid = grow < a.M;
      const int64_t smp = valid ? grow : a.M - 1;
      const float* src = a.obs + smp * D;
      const int nk0 = (D + 15) >> 4;
#pragma unroll
      for (int i = 0; i < MAXT; ++i)
        if (i < nk0) {
          const int col = 16 * i + ai;
          const float t = src[col < D ? col : 0];
          X[lrow * LDI + col] = (valid && col < D) ? t : 0.f;
        }
    }
    __syncthreads();

    // ---- 2: forward (and the tangent in product mode)
#pragma unroll
    for (int l = 0; l < NLAY; ++l) {
      const int in = net.dims[l], out = net.dims[l + 1];
      const float* IN = l == 0 ? X : H + (l - 1) * IMG;
#pragma unroll
      for (int s = 0; s < VW; ++s) {
      const Unit u = unit_of(wave + 4 * s, (out + 15) >> 4);
      if (u.on) {
        const int f0 = 16 * u.t + 4 * q;
        f4 h[2];
        if (MODE != M_FVP || l < NL) {
          h[0] = h[1] = bias4(a.theta + net.b[l], f0, out);
          mm_rows(a.theta + net.w[l], out, in, IN, u, j, q, h);
#pragma unroll
          for (int i = 0; i < 2; ++i)
            if (i < u.nr) {
              if (l < NL) {
                h[i] = fast_tanh4(h[i]);
                *reinterpret_cast<f4*>(H + l * IMG + (16 * (u.r0 + i) + j) * LDI + f0) = h[i];
              } else {
                *reinterpret_cast<f4*>(O + (16 * (u.r0 + i) + j) * LDO + f0) = h[i];
              }
            }
        }
        if (MODE == M_FVP) {
          f4 t[2];
          t[0] = t[1] = bias4(a.vec + net.b[l], f0, out);
          __builtin_amdgcn_sched_barrier(0);
          mm_rows(a.vec + net.w[l], out, in, IN, u, j, q, t);
          __builtin_amdgcn_sched_barrier(0);
          if (l > 0) mm_rows(a.theta + net.w[l], out, in, TB + ((l - 1) & 1) * IMG, u, j, q, t);
#pragma unroll
          for (int i = 0; i < 2; ++i)
            if (i < u.nr) {
              if (l < NL) {
#pragma unroll
                for (int r = 0; r < 4; ++r) t[i][r] *= fmaf(-h[i][r], h[i][r], 1.f);
                *reinterpret_cast<f4*>(TB + (l & 1) * IMG + (16 * (u.r0 + i) + j) * LDI + f0) = t[i];
              } else {
                *reinterpret_cast<f4*>(O + (16 * (u.r0 + i) + j) * LDO + f0) = t[i];
              }
            }
        }
      }
      __builtin_amdgcn_sched_barrier(0);            // one virtual wave's fragments at a time
      }
      __syncthreads();
    }

    // ---- NL + 3: the loss at the output, one (row, action slot) per thread
#pragma unroll
    for (int hh = 0; hh < ROWS * 16 / NTHR; ++hh) {
      const int lrow = (tid >> 4) + hh * (NTHR / 16);
      const int64_t grow = c * ROWS + lrow;
      const bool valid = grow < a.M;
      const int64_t smp = valid ? grow : a.M - 1;
      const float o = O[lrow * LDO + ai];
      if (MODE == M_SURR) {
        const float t = a.act[smp * A + (on ? ai : 0)];
        const float dif = (on ? t : 0.f) - o;
        float lp = -(dif * dif) * (0.5f * ivar) - lsd;
        lp += __shfl_xor(lp, 1); lp += __shfl_xor(lp, 2); lp += __shfl_xor(lp, 4); lp += __shfl_xor(lp, 8);
        const float ratio = expf(lp - a.logp_old[smp]);                  // cpo.py:358 / :374
        const float adv = a.adv[smp];
        if (ai == 0 && valid) lsum += (double)(ratio * adv);
        const float dlp = valid ? a.sign * adv * ratio * inv_m : 0.f;    // d(sign * mean(ratio * adv)) / dlogp
        const float z = dif * ivar;
        O[lrow * LDO + ai] = dlp * z;
        dls = fmaf(dlp * amask, dif * z - 1.f, dls);
      } else if (MODE == M_FVP) {
        O[lrow * LDO + ai] = o * ivar * amask * (valid ? inv_ma : 0.f);
      } else if (MODE == M_LS) {
        float lp = 0.f, kl = 0.f;
        if (on) {
          const float dif = a.act[smp * A + ai] - o;
          lp = -(dif * dif) * (0.5f * ivar) - lsd;
          const float rs = sdo / sdn;
          const float vr = rs * rs;
          const float dm = (a.mean_old[smp * A + ai] - o) / sdn;
          kl = 0.5f * (vr + dm * dm - 1.f - logf(vr));
        }
        lp += __shfl_xor(lp, 1); lp += __shfl_xor(lp, 2); lp += __shfl_xor(lp, 4); lp += __shfl_xor(lp, 8);
        const float ratio = expf(lp - a.logp_old[smp]);
        if (valid) {
          s_kl += (double)kl;
          if (ai == 0) { s_r += (double)(ratio * a.adv[smp]); s_c += (double)(ratio * a.adv2[smp]); }
        }
      } else {
        if (valid && on) a.mean_out[grow * A + ai] = o;
      }
    }
    __syncthreads();

    // ---- NL + 4 ..: backward
    if (GRAD) {
#pragma unroll
      for (int l = NL; l >= 0; --l) {
        const int in = net.dims[l], out = net.dims[l + 1];
        const int ntm = (out + 15) >> 4, ntk = (in + 15) >> 4;
        const float* DZ = l == NL ? O : TB + (l & 1) * IMG;
        const int ldz = l == NL ? LDO : LDI;
        const float* IN = l == 0 ? X : H + (l - 1) * IMG;
        const bool wide = ntm > 4;
#pragma unroll
        for (int s = 0; s < VW; ++s) {
        const int vw = wave + 4 * s;
        const int mt = wide ? vw : vw >> 1, k0 = wide ? 0 : vw & 1, ks = wide ? 1 : 2;
        if (mt < ntm) {
#pragma unroll
          for (int rt = 0; rt < 2; ++rt) {
            const int row0 = 16 * rt + 4 * q;
            float az[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) az[r] = DZ[(row0 + r) * ldz + 16 * mt + j];
            db[s][l] += (az[0] + az[1]) + (az[2] + az[3]);
            float bh[MAXT][4];
#pragma unroll
            for (int i = 0; i < MAXT; ++i)
              if (k0 + i * ks < ntk) {
#pragma unroll
                for (int r = 0; r < 4; ++r) bh[i][r] = IN[(row0 + r) * LDI + 16 * (k0 + i * ks) + j];
              }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
              for (int i = 0; i < MAXT; ++i)
                if (k0 + i * ks < ntk) {
                  if (l < NL) accW[s][l][i] = mfma4(az[r], bh[i][r], accW[s][l][i]);
                  else if (s == 0 && i < MAXT / 2) accO[i] = mfma4(az[r], bh[i][r], accO[i]);
                }
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        }
        __builtin_amdgcn_sched_barrier(0);          // the dH fragments stay out of the dW products' register budget
        if (l > 0) {
#pragma unroll
          for (int s = 0; s < VW; ++s) {
          const Unit u = unit_of(wave + 4 * s, ntk);
          if (u.on) {
            const float* Wg = a.theta + net.w[l];
            f4 af[MAXT];
#pragma unroll
            for (int nt = 0; nt < MAXT; ++nt)
              if (nt < ntm) af[nt] = ld_col4(Wg, in, 16 * nt + 4 * q, out, 16 * u.t + j, in);
            f4 acc[2] = {f4{0.f, 0.f, 0.f, 0.f}, f4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int nt = 0; nt < MAXT; ++nt)
              if (nt < ntm) {
                f4 b[2];
#pragma unroll
                for (int i = 0; i < 2; ++i)
                  if (i < u.nr) b[i] = *reinterpret_cast<const f4*>(DZ + (16 * (u.r0 + i) + j) * ldz + 16 * nt + 4 * q);
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                  for (int i = 0; i < 2; ++i)
                    if (i < u.nr) acc[i] = mfma4(af[nt][r], b[i][r], acc[i]);
              }
#pragma unroll
            for (int i = 0; i < 2; ++i)
              if (i < u.nr) {
                const int f = (16 * (u.r0 + i) + j) * LDI + 16 * u.t + 4 * q;
                const f4 hv = *reinterpret_cast<const f4*>(IN + f);
                f4 dz;
#pragma unroll
                for (int r = 0; r < 4; ++r) dz[r] = acc[i][r] * fmaf(-hv[r], hv[r], 1.f);
                *reinterpret_cast<f4*>(TB + ((l - 1) & 1) * IMG + f) = dz;
              }
          }
          __builtin_amdgcn_sched_barrier(0);
          }
        }
        __syncthreads();
      }
    }
  }

  // ---- this workgroup's partial vector / sums: every element written exactly once, sums in fixed order
  double* const redd = reinterpret_cast<double*>(lds);
  const int j = j0, q = q0;
  if (GRAD) {
    float* out = a.partial + (int64_t)blockIdx.x * net.Pa;
#pragma unroll
    for (int l = 0; l < NLAY; ++l) {
      const int in = net.dims[l], outw = net.dims[l + 1];
      const int ntm = (outw + 15) >> 4, ntk = (in + 15) >> 4;
      const bool wide = ntm > 4;
#pragma unroll
      for (int v = 0; v < VW; ++v) {
      const int vw = wave + 4 * v;
      const int mt = wide ? vw : vw >> 1, k0 = wide ? 0 : vw & 1, ks = wide ? 1 : 2;
      float s = db[v][l];
      s += __shfl_xor(s, 16);
      s += __shfl_xor(s, 32);
      if (mt < ntm) {
#pragma unroll
        for (int i = 0; i < MAXT; ++i) {
          const int k = 16 * (k0 + i * ks) + j;
          if (k0 + i * ks < ntk && k < in) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int m = 16 * mt + 4 * q + r;
              if (m < outw) out[net.w[l] + m * in + k] = l < NL ? accW[v][l][i][r] : accO[v == 0 && i < MAXT / 2 ? i : 0][r];
            }
          }
        }
        if (k0 == 0 && q == 0 && 16 * mt + j < outw) out[net.b[l] + 16 * mt + j] = s;
      }
      }
    }
    constexpr int NG = NTHR / 16;                       // 16-lane groups: one row of each half chunk
    float* const redf = lds + 2 * NG;                   // behind the doubles of the loss sum
    redf[tid] = dls;
    if (ai == 0) redd[tid >> 4] = lsum;
    __syncthreads();
    if (tid < A) {
      float s = 0.f;
      if (MODE == M_SURR)
        for (int r = 0; r < NG; ++r) s += redf[16 * r + tid];
      out[tid] = s;
    }
    if (tid == 0) {
      double s = 0.0;
      for (int r = 0; r < NG; ++r) s += redd[r];
      a.partial_loss[blockIdx.x] = s;
    }
  } else if (MODE == M_LS) {
    redd[tid] = s_kl;
    constexpr int NG = NTHR / 16;
    if (ai == 0) { redd[NTHR + (tid >> 4)] = s_r; redd[NTHR + NG + (tid >> 4)] = s_c; }
    __syncthreads();
    if (tid < 3) {
      double s = 0.0;
      if (tid == 2) for (int k = 0; k < NTHR; ++k) s += redd[k];
      else for (int r = 0; r < NG; ++r) s += redd[NTHR + tid * NG + r];
      a.ls_partials[blockIdx.x * 3 + tid] = s;
    }
  }
}

// out[i] = sum_k partial[k][i] in the order of k, sixteen loads in flight at a time (the scheme of cpo.hip's reduction)
__global__ __launch_bounds__(64) void cpo_rows_reduce_kernel(const float* partial, int nparts, int P, float* out, const double* ploss,
                                                             double* loss_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < P) {
    float acc = 0.f;
    int k = 0;
    for (; k + 16 <= nparts; k += 16) {
      float v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = partial[(int64_t)(k + u) * P + i];
#pragma unroll
      for (int u = 0; u < 16; ++u) acc += v[u];
    }
    for (; k < nparts; ++k) acc += partial[(int64_t)k * P + i];
    out[i] = acc;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && loss_out) {
    double l = 0.0;
    for (int k = 0; k < nparts; ++k) l += ploss[k];
    loss_out[0] = l;
  }
}

__global__ void cpo_rows_sum3_kernel(const double* partials, int n, double* out) {
  if (threadIdx.x < 3) {
    double s = 0;
    for (int k = 0; k < n; ++k) s += partials[k * 3 + threadIdx.x];
    out[threadIdx.x] = s;
  }
}

// the envelope; 0 and RowsNet filled in, or -1 / -2 with the dimension named
int make_net(const spo_mlp_net* net, RowsNet& rn) {
  SPO_REQUIRE(net, "cpo_rows: bad args (net is null)");
  const int n = net->n_layers;
  // three hidden layers (NL = 3) compile, but with 296-332 B of scratch per lane for the 256 + 16 accumulators: not shipped
  if (n != 3) return spo::fail(-2, "cpo_rows: %d hidden layers, the kernels take exactly 2", n - 1);
  if (net->dims[0] < 1 || net->dims[0] > MAXW) return spo::fail(-2, "cpo_rows: obs_dim %d outside [1,%d]", net->dims[0], MAXW);
  for (int l = 1; l < n; ++l)
    if (net->dims[l] < 1 || net->dims[l] > MAXW)
      return spo::fail(-2, "cpo_rows: hidden width %d of layer %d outside [1,%d]", net->dims[l], l, MAXW);
  if (net->dims[n] < 1 || net->dims[n] > MAXA) return spo::fail(-2, "cpo_rows: act_dim %d outside [1,%d]", net->dims[n], MAXA);
  rn = RowsNet{};
  rn.n = n;
  int off = net->dims[n];                            // log_std first
  for (int l = 0; l <= n; ++l) rn.dims[l] = net->dims[l];
  for (int l = 0; l < n; ++l) {
    rn.w[l] = off;
    off += net->dims[l + 1] * net->dims[l];
    rn.b[l] = off;
    off += net->dims[l + 1];
  }
  rn.Pa = off;
  return 0;
}

template <int NL, int MODE>
int launch_nl(const RowsArgs& a, int blocks, hipStream_t st) {
  constexpr size_t bytes = lds_floats<NL, MODE>() * sizeof(float);
  static_assert(bytes <= 160 * 1024, "cpo_rows: the chunk's images do not fit one workgroup's LDS");
  static_assert((NTHR + 2 * ROWS) * sizeof(double) <= bytes, "cpo_rows: the final sums reuse the images");
  static bool attr_done[spo::SPO_MAX_DEVICES] = {};
  return spo::launch_dyn_lds(&cpo_rows_kernel<NL, MODE>, attr_done, "cpo_rows", dim3(blocks), dim3(NTHR), bytes, st, a);
}

template <int MODE>
int launch(const RowsArgs& a, int blocks, hipStream_t st) {
  return launch_nl<2, MODE>(a, blocks, st);
}

}  // namespace

extern "C" int spo_cpo_rows_supported(const spo_mlp_net* net) {
  RowsNet rn;
  return (net && make_net(net, rn) == 0) ? 1 : 0;
}

extern "C" int spo_cpo_rows_chunk_rows(void) { return ROWS; }

extern "C" int spo_cpo_rows_num_partials(int64_t rows) {
  const int64_t n = (rows + ROWS - 1) / ROWS;
  return (int)(n < 1 ? 1 : n < MAX_GRID ? n : MAX_GRID);
}

extern "C" int spo_cpo_rows_surrogate_grad(const float* theta, const float* obs, const float* act, const float* logp_old,
                                           const float* adv, float sign, int64_t rows, const spo_mlp_net* net, float* partial_ws,
                                           double* loss_ws, float* grad_out, double* loss_sum_out, void* stream) {
  RowsArgs a{};
  if (int rc = make_net(net, a.net)) return rc;
  SPO_REQUIRE(theta && obs && act && logp_old && adv && partial_ws && loss_ws && grad_out && loss_sum_out && rows > 0,
              "cpo_rows_surrogate_grad: bad args");
  const int blocks = spo_cpo_rows_num_partials(rows);
  a.theta = theta; a.obs = obs; a.act = act; a.logp_old = logp_old; a.adv = adv; a.M = rows; a.sign = sign;
  a.partial = partial_ws; a.partial_loss = loss_ws;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = launch<M_SURR>(a, blocks, st)) return rc;
  hipLaunchKernelGGL(cpo_rows_reduce_kernel, dim3((a.net.Pa + 63) / 64), dim3(64), 0, st, partial_ws, blocks, a.net.Pa, grad_out,
                     loss_ws, loss_sum_out);
  SPO_LAUNCH_CHECK("spo_cpo_rows_surrogate_grad");
  return 0;
}

extern "C" int spo_cpo_rows_fvp(const float* theta, const float* obs, const float* vec, int64_t rows, const spo_mlp_net* net,
                                float* partial_ws, double* loss_ws, float* out, void* stream) {
  RowsArgs a{};
  if (int rc = make_net(net, a.net)) return rc;
  SPO_REQUIRE(theta && obs && vec && partial_ws && loss_ws && out && rows > 0, "cpo_rows_fvp: bad args");
  const int blocks = spo_cpo_rows_num_partials(rows);
  a.theta = theta; a.vec = vec; a.obs = obs; a.M = rows; a.sign = 1.f; a.partial = partial_ws; a.partial_loss = loss_ws;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = launch<M_FVP>(a, blocks, st)) return rc;
  hipLaunchKernelGGL(cpo_rows_reduce_kernel, dim3((a.net.Pa + 63) / 64), dim3(64), 0, st, partial_ws, blocks, a.net.Pa, out, loss_ws,
                     (double*)nullptr);
  SPO_LAUNCH_CHECK("spo_cpo_rows_fvp");
  return 0;
}

extern "C" int spo_cpo_rows_linesearch_eval(const float* theta, const float* obs, const float* act, const float* logp_old,
                                            const float* adv_r, const float* adv_c, const float* mean_old, const float* log_std_old,
                                            int64_t rows, const spo_mlp_net* net, double* partial_ws, int partial_capacity,
                                            double* sums3_out, void* stream) {
  RowsArgs a{};
  if (int rc = make_net(net, a.net)) return rc;
  SPO_REQUIRE(theta && obs && act && logp_old && adv_r && adv_c && mean_old && log_std_old && partial_ws && sums3_out && rows > 0,
              "cpo_rows_linesearch_eval: bad args");
  int blocks = spo_cpo_rows_num_partials(rows);
  if (blocks * 3 > partial_capacity) blocks = partial_capacity / 3;
  SPO_REQUIRE(blocks >= 1, "cpo_rows_linesearch_eval: partial capacity too small");
  a.theta = theta; a.obs = obs; a.act = act; a.logp_old = logp_old; a.adv = adv_r; a.adv2 = adv_c; a.mean_old = mean_old;
  a.log_std_old = log_std_old; a.M = rows; a.ls_partials = partial_ws;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = launch<M_LS>(a, blocks, st)) return rc;
  hipLaunchKernelGGL(cpo_rows_sum3_kernel, dim3(1), dim3(64), 0, st, partial_ws, blocks, sums3_out);
  SPO_LAUNCH_CHECK("spo_cpo_rows_linesearch_eval");
  return 0;
}

extern "C" int spo_cpo_rows_actor_mean(const float* theta, const float* obs, float* mean_out, int64_t rows, const spo_mlp_net* net,
                                       void* stream) {
  RowsArgs a{};
  if (int rc = make_net(net, a.net)) return rc;
  SPO_REQUIRE(theta && obs && mean_out && rows > 0, "cpo_rows_actor_mean: bad args");
  a.theta = theta; a.obs = obs; a.M = rows; a.mean_out = mean_out;
  if (int rc = launch<M_MEAN>(a, spo_cpo_rows_num_partials(rows), (hipStream_t)stream)) return rc;
  SPO_LAUNCH_CHECK("spo_cpo_rows_actor_mean");
  return 0;
}
