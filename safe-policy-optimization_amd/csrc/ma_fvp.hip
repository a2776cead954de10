// MACPO's Fisher-vector product J^T diag(m) J v for the multi-agent actor, hidden width <= 128, gfx950 (spo_ma_fvp).
//
// Reference: safepo/multi_agent/macpo.py:187-199 differentiates the mean KL twice; at theta = theta_old that Hessian is J^T M J
// (safepo/multi_agent/macpo.py of this package), which spo_ma_jvp + spo_ma_backward evaluate launch by launch (26 launches at
// two blocks).  Here one product is four launches: the fold's tangent (fn_fold_tangent_kernel), ma_fvp_kernel, the fixed-order
// reduction of the workgroups' partial vectors, and the fold's unfold (fn_unfold_grad_kernel).
// Envelope (spo_ma_fvp_supported): an actor, in_dim 1..128, hidden 1..128, out_dim 1..16, 1 or 2 blocks.
//
// The network is  xhat -> [Linear -> ELU -> LayerNorm] x NB -> Linear head, block 0 on the folded weights (ma_layout.h); its forward
// activations are the ones spo_ma_forward left in ws, nothing is recomputed (y_k is LOADED, not rebuilt from a_k and the statistics).
//
// Grid: at most 256 workgroups of 256 threads = 4 waves, each playing two of eight "virtual waves" (rows_frag.h); workgroup b walks
// the 32-row chunks b, b + gridDim, ...  Weights and the direction are read as v_mfma_f32_16x16x4_f32 (exact fp32) A fragments
// straight from global memory / L2.  LDS holds the chunk as ROW images [32][132]:
//
//   X            xhat, zero beyond in_dim                                                     32 x 132
//   A[k], Y[k]   post-ELU values and block outputs of block k, zero beyond hidden           32 x 132 each
//   TB[0], TB[1] forward: dz_k, then dy_k in place, in TB[k & 1]; backward: dy_k, then dz_k in place      32 x 132 each
//   O            the head's tangent times m (rows past the batch: zero)                       32 x 20
//   ST[k], RM    mean / rstd of the chunk's rows per block; the two row means of a LayerNorm backward     32 x 2 each
//   NB = 2: 7 x 16 896 + 2 560 + 768 = 121 600 B;  NB = 1: 87 552 B.
//
// Sub-phases of one chunk, one barrier after each:
//   1          the images <- ws (float4 per lane where the width allows)
//   per block  T   dz = tb + tW IN (+ W dy_{k-1}) on the feature-tile owners (tile w, both row tiles; hidden <= 64: tile w / 2,
//                  row tile w & 1)
//              LT  the LayerNorm tangent needs two means over a row whose tiles different waves own: 8 lanes per row read the
//                  row image, da = ELU'(a) dz, fixed-order lane reduction (xor 1, 2, 4), dy written in place
//   head       O = (thb + thW y + hW dy) m, zero for rows past the batch: every later row term of such a row is then zero
//   backward, layer l = NB .. 0:
//              W   dW_l += dz_l^T IN_l in MFMA accumulators on the band owners, and dy_{l-1} = dz_l W_l with the forward's split
//              LR  l > 0: the two row means of the LayerNorm backward, 8 lanes per row, into RM
//              LC  l > 0: thread = (feature, half of the rows): dg += dy xhat, dbe += dy, dz = ELU'(a) rstd (g dy - m1 - xhat m2)
//                  in place, db += dz: three registers per block instead of a row owner's 48
// Weight gradients never leave the accumulators inside the chunk loop (virtual wave w owns the 16-row band w of dW'_0 and dW_1:
// 2 x 32 registers per block and wave, 16 for the head, 144 at NB = 2).  After the last chunk the workgroup writes ONE partial
// vector laid out like theta, every element exactly once (the input LayerNorm's and log_std's slots as zeros).  No atomics:
// repeats are bit-identical.
#include "common.h"
#include "rows_frag.h"
#include "ma_layout.h"

namespace {
using namespace spo;
using namespace spo::rows;

constexpr int MAXB = 2;                    // blocks

struct FvpArgs {
  int D, H, O;
  int64_t B;
  float rows_global;
  int vec4;                                // ws is 16-byte aligned: the float4 loads of the images
  const float* theta; const float* vec; const float* m_diag; const float* tWf; const float* tbf;
  const float* xhat; const float* a[MAXB]; const float* st[MAXB]; const float* y[MAXB];
  int w[MAXB + 1], b[MAXB + 1], g[MAXB], be[MAXB], logstd;      // offsets in theta; index NB: the head
  int P;
  float* partial;
};

template <int NB>
constexpr int lds_floats() { return (3 + 2 * NB) * IMG + ROWS * LDO + (NB + 1) * ROWS * 2; }

template <int NB>
__global__ __launch_bounds__(NTHR, 1) void ma_fvp_kernel(FvpArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  float* const X = lds;
  float* const A = lds + IMG;
  float* const Y = lds + (1 + NB) * IMG;
  float* const TB = lds + (1 + 2 * NB) * IMG;
  float* const O = lds + (3 + 2 * NB) * IMG;
  float* const ST = O + ROWS * LDO;
  float* const RM = ST + NB * ROWS * 2;
  const int D = a.D, H = a.H, Od = a.O;
  const int nth = (H + 15) >> 4, Hp = 16 * nth;
  const float inv_h = 1.f / (float)H;
  // the row sub-phases: 8 lanes per row, lane s8 takes columns 32 i + 4 s8 .. + 3;  the column sub-phase: one feature, 16 rows
  const int chalf = wave >> 1;

  f4 accW[VW][NB][MAXT];
  f4 accO[MAXT / 2];                       // the head is one band: virtual waves 0 and 1, every other tile
  float dhb = 0.f;
  float cg[NB], cb[NB], cz[NB];            // this thread's feature: d(ln weight), d(ln bias), d(linear bias) of block k
#pragma unroll
  for (int k = 0; k < NB; ++k) {
    cg[k] = cb[k] = cz[k] = 0.f;
#pragma unroll
    for (int s = 0; s < VW; ++s)
#pragma unroll
      for (int i = 0; i < MAXT; ++i) accW[s][k][i] = f4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int i = 0; i < MAXT / 2; ++i) accO[i] = f4{0.f, 0.f, 0.f, 0.f};

  const int64_t nchunks = (a.B + ROWS - 1) / ROWS;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    // the lane coordinates are derived from an opaque copy of the thread index once per chunk: every fragment address and bounds
    // mask below depends on them, and hoisted out of the chunk loop as loop invariants they would take more registers than the
    // accumulators
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
    __syncthreads();

    // ---- forward tangent
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      const int in = k == 0 ? D : H;
      const float* IN = k == 0 ? X : Y + (k - 1) * IMG;
      const float* Wt = k == 0 ? a.tWf : a.vec + a.w[k];
      const float* bt = k == 0 ? a.tbf : a.vec + a.b[k];
      float* const T = TB + (k & 1) * IMG;
#pragma unroll
      for (int s = 0; s < VW; ++s) {
        const Unit u = unit_of(wave + 4 * s, nth);
        if (u.on) {
          const int f0 = 16 * u.t + 4 * q;
          f4 t[2];
          t[0] = t[1] = bias4(bt, f0, H);
          __builtin_amdgcn_sched_barrier(0);
          mm_rows(Wt, H, in, IN, u, j, q, t);
          __builtin_amdgcn_sched_barrier(0);
          if (k > 0) mm_rows(a.theta + a.w[k], H, H, TB + ((k - 1) & 1) * IMG, u, j, q, t);
#pragma unroll
          for (int i = 0; i < 2; ++i)
            if (i < u.nr) *reinterpret_cast<f4*>(T + (16 * (u.r0 + i) + j) * LDI + f0) = t[i];
        }
        __builtin_amdgcn_sched_barrier(0);            // one virtual wave's fragments at a time
      }
      __syncthreads();
      // LT: dy = tg xhat + g rstd (da - mean(da) - xhat mean(xhat da)) + tbe.  Columns H .. Hp hold dz = 0 and get dy = 0.
      {
        const float mean = ST[(k * ROWS + rrow) * 2], rstd = ST[(k * ROWS + rrow) * 2 + 1];
        float* const tr = T + rrow * LDI;
        const float* ar = A + k * IMG + rrow * LDI;
        f4 da[4], xh[4];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int c0 = 32 * i + 4 * s8;
          da[i] = xh[i] = f4{0.f, 0.f, 0.f, 0.f};
          if (c0 < Hp) {
            const f4 dz = *reinterpret_cast<const f4*>(tr + c0), av = *reinterpret_cast<const f4*>(ar + c0);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              da[i][e] = dz[e] * elu_grad(av[e]);
              xh[i][e] = (av[e] - mean) * rstd;
              s1 += da[i][e]; s2 += da[i][e] * xh[i][e];
            }
          }
        }
        const float m1 = sum8(s1) * inv_h, m2 = sum8(s2) * inv_h;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int c0 = 32 * i + 4 * s8;
          if (c0 < Hp) {
            const f4 g4 = bias4(a.theta + a.g[k], c0, H), tg4 = bias4(a.vec + a.g[k], c0, H), tbe4 = bias4(a.vec + a.be[k], c0, H);
            f4 dy;
#pragma unroll
            for (int e = 0; e < 4; ++e) dy[e] = tg4[e] * xh[i][e] + g4[e] * (rstd * (da[i][e] - m1 - xh[i][e] * m2)) + tbe4[e];
            *reinterpret_cast<f4*>(tr + c0) = dy;
          }
        }
      }
      __syncthreads();
    }

    // ---- head: dout = (thb + thW y + hW dy) m
#pragma unroll
    for (int s = 0; s < VW; ++s) {
      const Unit u = unit_of(wave + 4 * s, 1);
      if (u.on) {
        const int f0 = 4 * q;
        f4 t[2];
        t[0] = t[1] = bias4(a.vec + a.b[NB], f0, Od);
        __builtin_amdgcn_sched_barrier(0);
        mm_rows(a.vec + a.w[NB], Od, H, Y + (NB - 1) * IMG, u, j, q, t);
        __builtin_amdgcn_sched_barrier(0);
        mm_rows(a.theta + a.w[NB], Od, H, TB + ((NB - 1) & 1) * IMG, u, j, q, t);
        const f4 md = bias4(a.m_diag, f0, Od);
        const int lrow = 16 * u.r0 + j;
        const bool valid = row0 + lrow < a.B;
#pragma unroll
        for (int r = 0; r < 4; ++r) t[0][r] = valid ? t[0][r] * (md[r] / a.rows_global) : 0.f;
        *reinterpret_cast<f4*>(O + lrow * LDO + f0) = t[0];
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();

    // ---- backward
#pragma unroll
    for (int l = NB; l >= 0; --l) {
      const int in = l == 0 ? D : H, out = l == NB ? Od : H;
      const int ntm = (out + 15) >> 4, ntk = (in + 15) >> 4;
      const float* DZ = l == NB ? O : TB + (l & 1) * IMG;
      const int ldz = l == NB ? LDO : LDI;
      const float* IN = l == 0 ? X : Y + (l - 1) * IMG;
      const bool wide = ntm > 4;
      // W: the weight gradient on the band owners: band mt of 16 output features, tiles kt = k0 + i * ks of 16 input features
#pragma unroll
      for (int s = 0; s < VW; ++s) {
        const int vw = wave + 4 * s;
        const int mt = wide ? vw : vw >> 1, k0 = wide ? 0 : vw & 1, ks = wide ? 1 : 2;
        if (mt < ntm) {
#pragma unroll
          for (int rt = 0; rt < 2; ++rt) {
            const int r0 = 16 * rt + 4 * q;
            float az[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) az[r] = DZ[(r0 + r) * ldz + 16 * mt + j];
            if (l == NB && s == 0) dhb += (az[0] + az[1]) + (az[2] + az[3]);
            float bh[MAXT][4];
#pragma unroll
            for (int i = 0; i < MAXT; ++i)
              if (k0 + i * ks < ntk) {
#pragma unroll
                for (int r = 0; r < 4; ++r) bh[i][r] = IN[(r0 + r) * LDI + 16 * (k0 + i * ks) + j];
              }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
              for (int i = 0; i < MAXT; ++i)
                if (k0 + i * ks < ntk) {
                  if (l < NB) accW[s][l < NB ? l : 0][i] = mfma4(az[r], bh[i][r], accW[s][l < NB ? l : 0][i]);
                  else if (s == 0 && i < MAXT / 2) accO[i] = mfma4(az[r], bh[i][r], accO[i]);
                }
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      __builtin_amdgcn_sched_barrier(0);          // the dy fragments stay out of the dW products' register budget
      if (l > 0) {
        float* const DY = TB + ((l - 1) & 1) * IMG;
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
        float* const DY = TB + (kk & 1) * IMG;
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
            cg[kk] += dy * xh; cb[kk] += dy;
            const float dz = rstd * (dy * gc - m1 - xh * m2) * elu_grad(av);
            cz[kk] += dz;
            DY[row * LDI + ccol] = dz;
          }
        }
        __syncthreads();
      }
    }
  }

  // ---- this workgroup's partial vector: every element written exactly once
  const int j = tid & 15, q = (tid >> 4) & 3, ccol0 = tid & (MAXW - 1);
  float* out = a.partial + (int64_t)blockIdx.x * a.P;
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
              if (m < outw) out[a.w[l] + m * in + k] = l < NB ? accW[v][l < NB ? l : 0][i][r] : accO[v == 0 && i < MAXT / 2 ? i : 0][r];
            }
          }
        }
      }
    }
  }
  {
    float s = dhb;                                  // waves 0 and 1 both hold the head's band; wave 0 writes it
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 32);
    if (wave == 0 && q == 0 && j < Od) out[a.b[NB] + j] = s;
  }
  // the two halves' feature sums, half 0 first
  float* const red = lds;
  if (chalf == 1) {
#pragma unroll
    for (int k = 0; k < NB; ++k) { red[(3 * k) * MAXW + ccol0] = cg[k]; red[(3 * k + 1) * MAXW + ccol0] = cb[k]; red[(3 * k + 2) * MAXW + ccol0] = cz[k]; }
  }
  __syncthreads();
  if (chalf == 0 && ccol0 < H) {
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      out[a.g[k] + ccol0] = cg[k] + red[(3 * k) * MAXW + ccol0];
      out[a.be[k] + ccol0] = cb[k] + red[(3 * k + 1) * MAXW + ccol0];
      out[a.b[k] + ccol0] = cz[k] + red[(3 * k + 2) * MAXW + ccol0];
    }
  }
  for (int i = tid; i < 2 * D; i += NTHR) out[i] = 0.f;              // the input LayerNorm: filled by the unfold
  if (tid < Od) out[a.logstd + tid] = 0.f;
}

// out[i] = sum_k partial[k][i] in the order of k, sixteen loads in flight at a time
__global__ __launch_bounds__(64) void ma_fvp_reduce_kernel(const float* __restrict__ partial, int nparts, int P, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
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

// the envelope; 0, or -1 / -2 with the dimension named
int fvp_lay(const spo_ma_net* net, Lay* L) {
  if (int rc = lay_of(net, L)) return rc;
  if (!L->actor) return fail(-2, "ma_fvp: is_actor 0, the kernel takes an actor (the critics have no Fisher-vector product)");
  if (L->H > MAXW) return fail(-2, "ma_fvp: hidden %d outside [1,%d]", L->H, MAXW);
  if (L->D > MAXW) return fail(-2, "ma_fvp: in_dim %d outside [1,%d]", L->D, MAXW);
  if (L->O > MAXA) return fail(-2, "ma_fvp: out_dim %d outside [1,%d]", L->O, MAXA);
  if (L->NB > MAXB) return fail(-2, "ma_fvp: n_blocks %d outside [1,%d]", L->NB, MAXB);
  return 0;
}

int num_partials(int64_t rows) {
  const int64_t n = (rows + ROWS - 1) / ROWS;
  return (int)(n < 1 ? 1 : n < MAX_GRID ? n : MAX_GRID);
}

template <int NB>
int launch(const FvpArgs& a, int blocks, hipStream_t st) {
  constexpr size_t bytes = lds_floats<NB>() * sizeof(float);
  static_assert(bytes <= 160 * 1024, "ma_fvp: the chunk's images do not fit one workgroup's LDS");
  static_assert(3 * MAXB * MAXW <= IMG, "ma_fvp: the final sums reuse the first image");
  static bool attr_done[SPO_MAX_DEVICES] = {};
  return launch_dyn_lds(&ma_fvp_kernel<NB>, attr_done, "ma_fvp", dim3(blocks), dim3(NTHR), bytes, st, a);
}

}  // namespace

extern "C" int spo_ma_fvp_supported(const spo_ma_net* net) {
  Lay L;
  return (net && fvp_lay(net, &L) == 0) ? 1 : 0;
}

extern "C" int spo_ma_fvp_num_partials(int64_t rows) { return num_partials(rows); }

// scratch: the fold's tangent tW'[H, D], tb'[H], then one partial vector per workgroup
extern "C" int64_t spo_ma_fvp_scratch_floats(const spo_ma_net* net, int64_t rows) {
  Lay L;
  if (fvp_lay(net, &L) || rows < 1) return -1;
  return Lay::al4((int64_t)L.H * L.D) + Lay::al4(L.H) + (int64_t)num_partials(rows) * L.count();
}

extern "C" int spo_ma_fvp(const float* theta, const spo_ma_net* net, const float* vec, const float* m_diag, int64_t rows,
                          int64_t rows_global, const float* ws, float* scratch, float* out, void* stream) {
  Lay L;
  if (int rc = fvp_lay(net, &L)) return rc;
  SPO_REQUIRE(theta && vec && m_diag && ws && scratch && out, "ma_fvp: bad args (null pointer)");
  SPO_REQUIRE(rows > 0 && rows_global >= rows, "ma_fvp: bad args (rows %lld, rows_global %lld)", (long long)rows, (long long)rows_global);
  hipStream_t st = (hipStream_t)stream;
  const int64_t B = rows;
  float* tWf = scratch;
  float* tbf = tWf + Lay::al4((int64_t)L.H * L.D);
  float* partial = tbf + Lay::al4(L.H);
  FvpArgs a{};
  a.D = L.D; a.H = L.H; a.O = L.O; a.B = B; a.rows_global = (float)rows_global;
  a.vec4 = reinterpret_cast<uintptr_t>(ws) % 16 == 0;
  a.theta = theta; a.vec = vec; a.m_diag = m_diag; a.tWf = tWf; a.tbf = tbf;
  a.xhat = ws + L.ws_xhat();
  for (int k = 0; k < L.NB; ++k) {
    a.a[k] = ws + L.ws_a(B, k); a.st[k] = ws + L.ws_st(B, k); a.y[k] = ws + L.ws_y(B, k);
    a.w[k] = (int)L.W(k); a.b[k] = (int)L.b(k); a.g[k] = (int)L.g(k); a.be[k] = (int)L.be(k);
  }
  a.w[L.NB] = (int)L.hW(); a.b[L.NB] = (int)L.hb(); a.logstd = (int)L.logstd();
  a.P = (int)L.count();
  a.partial = partial;
  const int blocks = num_partials(B);
  hipLaunchKernelGGL(fn_fold_tangent_kernel, dim3(L.H), dim3(64), 0, st, theta + L.W(0), theta + L.fn_g(), theta + L.fn_b(),
                     vec + L.W(0), vec + L.b(0), vec + L.fn_g(), vec + L.fn_b(), L.H, L.D, tWf, tbf);
  if (int rc = L.NB == 1 ? launch<1>(a, blocks, st) : launch<2>(a, blocks, st)) return rc;
  hipLaunchKernelGGL(ma_fvp_reduce_kernel, dim3((a.P + 63) / 64), dim3(64), 0, st, partial, blocks, a.P, out);
  // out + W(0) holds dW' = dz_0^T xhat: turn it into dW_0 and read the input LayerNorm's two gradients off it
  hipLaunchKernelGGL(fn_unfold_grad_kernel, dim3((L.D + 63) / 64), dim3(64), 0, st, theta + L.W(0), theta + L.fn_g(), theta + L.fn_b(),
                     out + L.W(0), out + L.b(0), L.H, L.D, out + L.fn_g(), out + L.fn_b());
  SPO_LAUNCH_CHECK("spo_ma_fvp");
  return 0;
}
