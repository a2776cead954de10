// CPO full-batch actor kernels, gfx950.
//
// Reference: safepo/single_agent/cpo.py
//   :356-365, :372-381  policy-gradient pair  g = -grad(-mean(ratio*adv_r)),  b = grad(mean(ratio*adv_c))
//   :132-157            fvp(): Hessian of mean(KL(old || cur)) over rows AND action dims at cur == old, times v,
//                       + 0.1*v (double backward over the full batch in the reference, 33 times per epoch)
//   :465-519            line search: loss_reward, loss_cost, KL for a candidate parameter vector
//   :534-571            critic fit (minibatch loop; runs on the persistent kernel of update.hip)
//
// One kernel, two modes, many workgroups: each workgroup walks 64-row chunks of the batch
// (chunk = blockIdx, += gridDim), accumulating weight-gradient tiles in MFMA accumulators across
// all its chunks, then writes ONE partial flat vector; a second kernel sums the partials in a
// fixed order (deterministic, no atomics).
//   MODE_SURR: forward, ratio = exp(logp - logp_old), dL/dlogp = sign*adv*ratio/M, backward.
//   MODE_FVP : forward, forward-mode tangent J v through the MLP (second LDS image holds v laid out
//              like the weights), cotangent u = (J v) / sigma^2 / (M*A), backward  ->  J^T u.
//              For a diagonal Gaussian with state-independent log_std the Hessian of the mean KL at
//              cur == old is block diagonal: J^T diag(1/sigma^2) J / (M*A) on the mean network and
//              2/A on log_std (added on the host together with the 0.1 damping).
//
// obs_dim 65..128 (KIN = 128; the spo_cpo128_* entry points): the surrogate form and the line search are instantiations of
// the same kernels (147 776 B and 56 128 B of LDS).  MODE_FVP's second network image does not fit beside the five
// transposed buffers (203 904 B of 163 840), so the product has a layout of its own:
//   MODE_FVP_REUSE: both images + THREE buffers P (64 x 68), Q (64 x 68), R (16 x 68) = 151 680 B, reused by four sub-phases
//              1  P = H1^T, Q = dZ2^T, R = dO^T          -> dW2, db2
//              2  P = H2^T, Q = dZ1^T                    -> dW3, db3; this wave's dZ1^T rows go to registers, db1
//              3  P = X^T features 0..63                 -> dW1 columns 0..63
//              4  P = X^T features 64..127               -> dW1 columns 64..127
//   with x kept in registers until sub-phases 3 / 4.  Eight barriers per chunk instead of four, one forward pass, no global
//   round trip; every accumulator receives the same products in the same order as in MODE_FVP (bit-identical to the two-launch
//   form that was measured against it: DESIGN_NOTES.md).
//
// obs_dim 129..512, act_dim 1..32 (HumanoidVelocity; the spo_cpo512_* entry points): neither W1 (99 KB at 384 features) nor a
// second image fits, and the kernels above assume one 16-row output tile.  Kernels of their own at the end of this file, on the
// same grid / partial-vector / fixed-order-reduction structure: W1 streamed through P / Q in 64-feature slices, two output tiles.
#include "common.h"
#include "mlp_mfma.h"
#include "../../include/safepo_hip.h"

namespace {
using namespace spo;

constexpr int LDB = 64 + 4;
enum { MODE_SURR = 0, MODE_FVP = 1, MODE_FVP_REUSE = 2 };

template <int KIN, int MODE>
struct CpoLds {
  using L = NetLds<KIN>;
  static constexpr int W = 0;
  static constexpr int V = L::SIZE;                               // FVP only
  static constexpr bool REUSE = MODE == MODE_FVP_REUSE;           // P = XT = H1T = H2T, Q = DZT, R = DOT
  static constexpr int XT = (MODE == MODE_SURR ? 1 : 2) * L::SIZE;
  static constexpr int H1T = REUSE ? XT : XT + KIN * LDB;
  static constexpr int H2T = REUSE ? XT : H1T + HID * LDB;
  static constexpr int DZT = H2T + HID * LDB;                     // dZ2^T, then dZ1^T (two sub-phases)
  static constexpr int DOT = DZT + HID * LDB;
  static constexpr int RED = DOT + OUTP * LDB;
  static constexpr int SIZE = RED + 64;
};

struct CpoArgs {
  const float* theta;        // full flat parameter vector (actor segment is used)
  const float* vec;          // FVP: direction, flat ACTOR layout [log_std, W1, b1, W2, b2, W3, b3]
  const float* obs; const float* act; const float* logp_old; const float* adv;
  int64_t M; int D; int A; float sign;
  float* partial;            // [gridDim][Pa]
  double* partial_loss;      // [gridDim]
};

template <int KIN, int MODE>
__global__ __launch_bounds__(256, 1) void cpo_actor_kernel(CpoArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  using U = CpoLds<KIN, MODE>;
  using L = NetLds<KIN>;
  constexpr int NT1 = KIN / 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, q = lane >> 4;
  const int D = a.D, A = a.A;
  const NetGeom g = net_geom(D, A, 2);
  const int ls_off = g.off - A;
  const int Pa = actor_size(D, A);
  stage_net<KIN>(a.theta, g, lds + U::W, tid, 256);
  if (MODE != MODE_SURR) {
    // the direction vector uses the actor's own flat layout: shift it so that net_geom offsets apply
    NetGeom gv = g;
    gv.off = A;                                   // W1 of the direction sits after its log_std block
    __syncthreads();
    stage_net<KIN>(a.vec, gv, lds + U::V, tid, 256);
  }
  __syncthreads();
  const float* Wl = lds + U::W;
  const float* Vl = lds + U::V;
  float* const red = lds + U::RED;

  float ivar[4], lsd[4], amask[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int ai = 4 * q + r;
    const bool on = ai < A;
    const float lsv = on ? a.theta[ls_off + ai] : 0.f;
    const float sdv = expf(lsv);
    amask[r] = on ? 1.f : 0.f;
    ivar[r] = 1.f / (sdv * sdv);
    lsd[r] = on ? lsv + LOG_SQRT_2PI : 0.f;
  }
  const int orow = 16 * wave + 4 * q;
  const int mycol = 16 * wave + j;
  f4 aW1[NT1], aW2[4], aW3 = {0.f, 0.f, 0.f, 0.f}, dls = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int nt = 0; nt < NT1; ++nt) aW1[nt] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) aW2[nt] = f4{0.f, 0.f, 0.f, 0.f};
  float db1 = 0.f, db2 = 0.f, db3 = 0.f;
  double lsum = 0.0;
  const float inv_m = (float)(1.0 / (double)a.M);
  const float inv_ma = (float)(1.0 / ((double)a.M * (double)A));

  const int64_t nchunks = (a.M + 63) / 64;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int64_t row = c * 64 + mycol;
    const bool cv = row < a.M;
    const int64_t smp = cv ? row : a.M - 1;
    f4 x[NT1];
    load_obs_tiles<KIN>(a.obs + smp * D, D, q, x);
    if (MODE != MODE_FVP_REUSE) {
#pragma unroll
      for (int nt = 0; nt < NT1; ++nt)
#pragma unroll
        for (int e = 0; e < 4; ++e) lds[U::XT + (16 * nt + 4 * q + e) * LDB + mycol] = x[nt][e];
    }
    f4 h1[4], h2[4];
    const f4 o = net_forward<KIN>(Wl, x, h1, h2, j, q);
    f4 dO = {0.f, 0.f, 0.f, 0.f};
    if (MODE == MODE_SURR) {
      float lp = 0.f, dif[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ai = 4 * q + r;
        const float t = a.act[smp * A + (ai < A ? ai : 0)];
        dif[r] = (ai < A ? t : 0.f) - o[r];
        lp += -(dif[r] * dif[r]) * (0.5f * ivar[r]) - lsd[r];
      }
      lp += __shfl_xor(lp, 16);
      lp += __shfl_xor(lp, 32);
      const float ratio = expf(lp - a.logp_old[smp]);                 // cpo.py:358 / :374
      const float adv = a.adv[smp];
      if (q == 0 && cv) lsum += (double)(ratio * adv);
      const float dlp = cv ? a.sign * adv * ratio * inv_m : 0.f;      // d(sign*mean(ratio*adv))/dlogp
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float z = dif[r] * ivar[r];
        dO[r] = dlp * z;
        dls[r] = fmaf(dlp * amask[r], dif[r] * z - 1.f, dls[r]);
      }
    } else {
      // tangent (forward-mode) pass: t1 = V1 x + vb1 ; h1' = (1-h1^2) t1 ; t2 = W2 h1' + V2 h1 + vb2 ; ...
      // KIN = 128: scheduling fences between the layers keep each layer's operand reads out of the previous layer's register
      // budget (119 instead of 155 AGPRs used as spill space); the narrower forms are scheduled as before
      constexpr bool FENCE = KIN > 64;
      f4 t1[4], t2[4];
      if (FENCE) __builtin_amdgcn_sched_barrier(0);
      layer_hidden<NT1, false>(Vl + L::W1, L::LD1, Vl + L::B1, x, t1, j, q);
      if (FENCE) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) t1[mt][r] *= fmaf(-h1[mt][r], h1[mt][r], 1.f);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) t2[mt] = *reinterpret_cast<const f4*>(Vl + L::B2 + 16 * mt + 4 * q);
      layer_accum<4>(Wl + L::W2, LDH, t1, t2, j, q);
      if (FENCE) __builtin_amdgcn_sched_barrier(0);
      layer_accum<4>(Vl + L::W2, LDH, h1, t2, j, q);
      if (FENCE) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) t2[mt][r] *= fmaf(-h2[mt][r], h2[mt][r], 1.f);
      f4 mud = *reinterpret_cast<const f4*>(Vl + L::B3 + 4 * q);
      mud = out_accum(Wl + L::W3, t2, mud, j, q);
      mud = out_accum(Vl + L::W3, h2, mud, j, q);
      const float cm = cv ? inv_ma : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) dO[r] = mud[r] * ivar[r] * amask[r] * cm;
    }

    // ---- backward through the MLP
    f4 dz2[4], dz1[4];
    {
      f4 acc[4];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) acc[mt] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
          acc[mt] = mfma4(Wl[L::W3 + (4 * q + r) * LDH + 16 * mt + j], dO[r], acc[mt]);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) dz2[mt][r] = acc[mt][r] * fmaf(-h2[mt][r], h2[mt][r], 1.f);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) acc[mt] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int mt = 0; mt < 4; ++mt)
            acc[mt] = mfma4(Wl[L::W2 + (16 * nt + 4 * q + r) * LDH + 16 * mt + j], dz2[nt][r], acc[mt]);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) dz1[mt][r] = acc[mt][r] * fmaf(-h1[mt][r], h1[mt][r], 1.f);
    }

    if (MODE == MODE_FVP_REUSE) {
      constexpr int P = U::XT, Q = U::DZT, R = U::DOT;
      // 1: P = H1^T, Q = dZ2^T, R = dO^T  ->  dW2
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int f = (16 * mt + 4 * q + r) * LDB + mycol;
          lds[P + f] = h1[mt][r];
          lds[Q + f] = dz2[mt][r];
        }
#pragma unroll
      for (int r = 0; r < 4; ++r) lds[R + (4 * q + r) * LDB + mycol] = dO[r];
      __syncthreads();
      {
        f4 az[4];
        float rs = 0.f;
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          az[r4] = *reinterpret_cast<const f4*>(lds + Q + (16 * wave + j) * LDB + 16 * r4 + 4 * q);
          rs += (az[r4][0] + az[r4][1]) + (az[r4][2] + az[r4][3]);
        }
        db2 += rs;
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          f4 bh[4];
#pragma unroll
          for (int nt = 0; nt < 4; ++nt)
            bh[nt] = *reinterpret_cast<const f4*>(lds + P + (16 * nt + j) * LDB + 16 * r4 + 4 * q);
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) aW2[nt] = mfma4(az[r4][e], bh[nt][e], aW2[nt]);
        }
      }
      __syncthreads();
      // 2: P = H2^T, Q = dZ1^T  ->  dW3; dZ1^T rows of this wave go to registers
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int f = (16 * mt + 4 * q + r) * LDB + mycol;
          lds[P + f] = h2[mt][r];
          lds[Q + f] = dz1[mt][r];
        }
      __syncthreads();
      f4 az1[4];
      {
        float rs = 0.f;
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const f4 az = *reinterpret_cast<const f4*>(lds + R + j * LDB + 16 * r4 + 4 * q);
          rs += (az[0] + az[1]) + (az[2] + az[3]);
          const f4 bh = *reinterpret_cast<const f4*>(lds + P + (16 * wave + j) * LDB + 16 * r4 + 4 * q);
#pragma unroll
          for (int e = 0; e < 4; ++e) aW3 = mfma4(az[e], bh[e], aW3);
        }
        db3 += rs;
        rs = 0.f;
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          az1[r4] = *reinterpret_cast<const f4*>(lds + Q + (16 * wave + j) * LDB + 16 * r4 + 4 * q);
          rs += (az1[r4][0] + az1[r4][1]) + (az1[r4][2] + az1[r4][3]);
        }
        db1 += rs;
      }
      // 3, 4: P = X^T features 0..63, then 64..127  ->  dW1 halves
#pragma unroll
      for (int half = 0; half < NT1 / 4; ++half) {
        __syncthreads();
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int e = 0; e < 4; ++e) lds[P + (16 * nt + 4 * q + e) * LDB + mycol] = x[4 * half + nt][e];
        __syncthreads();
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          f4 bh[4];
#pragma unroll
          for (int nt = 0; nt < 4; ++nt)
            bh[nt] = *reinterpret_cast<const f4*>(lds + P + (16 * nt + j) * LDB + 16 * r4 + 4 * q);
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) aW1[4 * half + nt] = mfma4(az1[r4][e], bh[nt][e], aW1[4 * half + nt]);
        }
      }
      __syncthreads();
      continue;
    }
    // ---- sub-phase A: dW3 (dO^T, H2^T) and dW2 (dZ2^T, H1^T)
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = (16 * mt + 4 * q + r) * LDB + mycol;
        lds[U::H1T + f] = h1[mt][r];
        lds[U::H2T + f] = h2[mt][r];
        lds[U::DZT + f] = dz2[mt][r];
      }
#pragma unroll
    for (int r = 0; r < 4; ++r) lds[U::DOT + (4 * q + r) * LDB + mycol] = dO[r];
    __syncthreads();
    {
      f4 az[4];
      float rs = 0.f;
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        az[r4] = *reinterpret_cast<const f4*>(lds + U::DZT + (16 * wave + j) * LDB + 16 * r4 + 4 * q);
        rs += (az[r4][0] + az[r4][1]) + (az[r4][2] + az[r4][3]);
      }
      db2 += rs;
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        f4 bh[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
          bh[nt] = *reinterpret_cast<const f4*>(lds + U::H1T + (16 * nt + j) * LDB + 16 * r4 + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) aW2[nt] = mfma4(az[r4][e], bh[nt][e], aW2[nt]);
      }
      rs = 0.f;
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        az[r4] = *reinterpret_cast<const f4*>(lds + U::DOT + j * LDB + 16 * r4 + 4 * q);
        rs += (az[r4][0] + az[r4][1]) + (az[r4][2] + az[r4][3]);
        const f4 bh = *reinterpret_cast<const f4*>(lds + U::H2T + (16 * wave + j) * LDB + 16 * r4 + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) aW3 = mfma4(az[r4][e], bh[e], aW3);
      }
      db3 += rs;
    }
    __syncthreads();
    // ---- sub-phase B: dW1 (dZ1^T, X^T); the dZ buffer is reused
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) lds[U::DZT + (16 * mt + 4 * q + r) * LDB + mycol] = dz1[mt][r];
    __syncthreads();
    {
      f4 az[4];
      float rs = 0.f;
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        az[r4] = *reinterpret_cast<const f4*>(lds + U::DZT + (16 * wave + j) * LDB + 16 * r4 + 4 * q);
        rs += (az[r4][0] + az[r4][1]) + (az[r4][2] + az[r4][3]);
      }
      db1 += rs;
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        f4 bh[NT1];
#pragma unroll
        for (int nt = 0; nt < NT1; ++nt)
          bh[nt] = *reinterpret_cast<const f4*>(lds + U::XT + (16 * nt + j) * LDB + 16 * r4 + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int nt = 0; nt < NT1; ++nt) aW1[nt] = mfma4(az[r4][e], bh[nt][e], aW1[nt]);
      }
    }
    __syncthreads();
  }

  // ---- emit this workgroup's partial flat vector (actor layout) -- every element written exactly once
  db1 += __shfl_xor(db1, 16); db1 += __shfl_xor(db1, 32);
  db2 += __shfl_xor(db2, 16); db2 += __shfl_xor(db2, 32);
  db3 += __shfl_xor(db3, 16); db3 += __shfl_xor(db3, 32);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float t = dls[r];
    t += __shfl_xor(t, 1); t += __shfl_xor(t, 2); t += __shfl_xor(t, 4); t += __shfl_xor(t, 8);
    if (j == 0) red[wave * 4 * 4 + 4 * q + r] = t;      // [wave][16]
  }
  const double lw = wave_sum_d(lsum);
  __shared__ double lred[4];
  if (lane == 0) lred[wave] = lw;
  __syncthreads();
  float* out = a.partial + (int64_t)blockIdx.x * Pa;
  const int w1 = A, b1 = w1 + HID * D, w2 = b1 + HID, b2 = w2 + HID * HID, w3 = b2 + HID, b3 = w3 + A * HID;
#pragma unroll
  for (int nt = 0; nt < NT1; ++nt)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (16 * nt + j < D) out[w1 + (orow + r) * D + 16 * nt + j] = aW1[nt][r];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int r = 0; r < 4; ++r) out[w2 + (orow + r) * HID + 16 * nt + j] = aW2[nt][r];
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (4 * q + r < A) out[w3 + (4 * q + r) * HID + 16 * wave + j] = aW3[r];
  if (q == 0) { out[b1 + 16 * wave + j] = db1; out[b2 + 16 * wave + j] = db2; }
  if (wave == 0 && q == 0 && j < A) out[b3 + j] = db3;
  if (wave == 0 && j == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ai = 4 * q + r;
      if (ai < A) out[ai] = (red[ai] + red[16 + ai]) + (red[32 + ai] + red[48 + ai]);
    }
  }
  if (tid == 0) a.partial_loss[blockIdx.x] = (lred[0] + lred[1]) + (lred[2] + lred[3]);
}

// out[i] = post_scale * sum_k partial[k][i] (+ diag terms of the FVP on the host side); fixed order.
__global__ __launch_bounds__(256) void reduce_partials_kernel(const float* partial, int nparts, int P, float* out,
                                                              const double* ploss, double* loss_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < P) {
    // sequential in k (the order every earlier round used: bit-identical sums), but sixteen loads are in flight before the
    // first of them is added -- one exposed memory latency per sixteen partials instead of one per partial (61 -> ~8 us for
    // 256 partial vectors of 8 592 floats)
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

// Line-search evaluation (cpo.py:473-491): sums of ratio*adv_r, ratio*adv_c and KL(old||new) (over
// rows AND dims) for the candidate parameters in theta.
struct LsArgs {
  const float* theta; const float* obs; const float* act; const float* logp_old; const float* adv_r;
  const float* adv_c; const float* mean_old; const float* log_std_old; double* partials; int64_t M; int D; int A;
};
template <int KIN>
__global__ __launch_bounds__(256) void cpo_linesearch_kernel(LsArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[NetLds<KIN>::SIZE];
  __shared__ double red[4][3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, q = lane >> 4;
  const int D = a.D, A = a.A;
  stage_net<KIN>(a.theta, net_geom(D, A, 2), lds, tid, 256);
  __syncthreads();
  const int ls_off = 2 * critic_size(D);
  float ivar[4], lsd[4], sdn[4], sdo[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int ai = 4 * q + r;
    const bool on = ai < A;
    const float lsv = on ? a.theta[ls_off + ai] : 0.f;
    sdn[r] = expf(lsv);
    sdo[r] = on ? expf(a.log_std_old[ai]) : 1.f;
    ivar[r] = 1.f / (sdn[r] * sdn[r]);
    lsd[r] = on ? logf(sdn[r]) + LOG_SQRT_2PI : 0.f;
  }
  double s_r = 0, s_c = 0, s_kl = 0;
  const int64_t ntiles = (a.M + 15) / 16;
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wave; tile < ntiles; tile += (int64_t)gridDim.x * 4) {
    const int64_t row = tile * 16 + j;
    const bool valid = row < a.M;
    const int64_t rr = valid ? row : a.M - 1;
    f4 x[KIN / 16];
    load_obs_tiles<KIN>(a.obs + rr * D, D, q, x);
    f4 h1[4], h2[4];
    const f4 mu = net_forward<KIN>(lds, x, h1, h2, j, q);
    float lp = 0.f, kl = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ai = 4 * q + r;
      if (ai < A) {
        const float dif = a.act[rr * A + ai] - mu[r];
        lp += -(dif * dif) * (0.5f * ivar[r]) - lsd[r];
        const float ratio = sdo[r] / sdn[r];
        const float vr = ratio * ratio;
        const float dm = (a.mean_old[rr * A + ai] - mu[r]) / sdn[r];
        kl += 0.5f * (vr + dm * dm - 1.f - logf(vr));
      }
    }
    lp += __shfl_xor(lp, 16); lp += __shfl_xor(lp, 32);
    const float ratio = expf(lp - a.logp_old[rr]);
    if (valid) {
      s_kl += (double)kl;                       // every lane holds its own dims
      if (q == 0) { s_r += (double)(ratio * a.adv_r[rr]); s_c += (double)(ratio * a.adv_c[rr]); }
    }
  }
  s_r = wave_sum_d(s_r); s_c = wave_sum_d(s_c); s_kl = wave_sum_d(s_kl);
  if (lane == 0) { red[wave][0] = s_r; red[wave][1] = s_c; red[wave][2] = s_kl; }
  __syncthreads();
  if (tid < 3) a.partials[blockIdx.x * 3 + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}
__global__ void sum3_kernel(const double* partials, int n, double* out) {
  if (threadIdx.x < 3) {
    double s = 0;
    for (int k = 0; k < n; ++k) s += partials[k * 3 + threadIdx.x];
    out[threadIdx.x] = s;
  }
}

int pick_kin(int D) { return D <= 16 ? 16 : D <= 32 ? 32 : 64; }

template <int K, int MODE>
int launch_cpo_k(const CpoArgs& a, int blocks, hipStream_t st) {
  static bool attr_done[spo::SPO_MAX_DEVICES] = {};
  return spo::launch_dyn_lds(&cpo_actor_kernel<K, MODE>, attr_done, "cpo", dim3(blocks), dim3(256),
                             CpoLds<K, MODE>::SIZE * sizeof(float), st, a);
}

template <int MODE>
int launch_cpo(const CpoArgs& a, int blocks, hipStream_t st) {
  const int kin = pick_kin(a.D);
  return kin == 16 ? launch_cpo_k<16, MODE>(a, blocks, st) : kin == 32 ? launch_cpo_k<32, MODE>(a, blocks, st)
                                                                       : launch_cpo_k<64, MODE>(a, blocks, st);
}

template <int MODE>
int launch_cpo128(const CpoArgs& a, int blocks, hipStream_t st) {
  static_assert(CpoLds<128, MODE>::SIZE * sizeof(float) <= 160 * 1024, "cpo128: LDS form does not fit one workgroup");
  return launch_cpo_k<128, MODE>(a, blocks, st);
}

int check(int D, int A) {
  if (D < 1 || D > 64) return spo::fail(-2, "cpo: obs_dim %d outside [1,64]", D);
  if (A < 1 || A > SPO_MAX_ACT) return spo::fail(-2, "cpo: act_dim %d outside [1,16]", A);
  return 0;
}

int check128(int D, int A) {
  if (D < 65 || D > 128) return spo::fail(-2, "cpo128: obs_dim %d outside [65,128]", D);
  if (A < 1 || A > SPO_MAX_ACT) return spo::fail(-2, "cpo128: act_dim %d outside [1,16]", A);
  return 0;
}

}  // namespace

extern "C" int spo_cpo_num_partials(int64_t rows) {
  int64_t n = (rows + 63) / 64;
  return (int)(n < 256 ? n : 256);
}

extern "C" int spo_cpo_surrogate_grad(const float* theta, const float* obs, const float* act, const float* logp_old,
                                      const float* adv, float sign, int64_t rows, int obs_dim, int act_dim,
                                      float* partial_ws, double* loss_ws, float* grad_out, double* loss_sum_out,
                                      void* stream) {
  if (int rc = check(obs_dim, act_dim)) return rc;
  SPO_REQUIRE(theta && obs && act && logp_old && adv && partial_ws && loss_ws && grad_out && loss_sum_out && rows > 0,
              "cpo_surrogate_grad: bad args");
  const int blocks = spo_cpo_num_partials(rows);
  CpoArgs a{theta, nullptr, obs, act, logp_old, adv, rows, obs_dim, act_dim, sign, partial_ws, loss_ws};
  hipStream_t st = (hipStream_t)stream;
  if (int rc = launch_cpo<MODE_SURR>(a, blocks, st)) return rc;
  const int Pa = spo::actor_size(obs_dim, act_dim);
  hipLaunchKernelGGL(reduce_partials_kernel, dim3((Pa + 63) / 64), dim3(64), 0, st, partial_ws, blocks, Pa, grad_out,
                     loss_ws, loss_sum_out);
  SPO_LAUNCH_CHECK("spo_cpo_surrogate_grad");
  return 0;
}

extern "C" int spo_cpo_fvp(const float* theta, const float* obs, const float* vec, int64_t rows, int obs_dim,
                           int act_dim, float* partial_ws, double* loss_ws, float* out, void* stream) {
  if (int rc = check(obs_dim, act_dim)) return rc;
  SPO_REQUIRE(theta && obs && vec && partial_ws && loss_ws && out && rows > 0, "cpo_fvp: bad args");
  const int blocks = spo_cpo_num_partials(rows);
  CpoArgs a{theta, vec, obs, nullptr, nullptr, nullptr, rows, obs_dim, act_dim, 1.f, partial_ws, loss_ws};
  hipStream_t st = (hipStream_t)stream;
  if (int rc = launch_cpo<MODE_FVP>(a, blocks, st)) return rc;
  const int Pa = spo::actor_size(obs_dim, act_dim);
  hipLaunchKernelGGL(reduce_partials_kernel, dim3((Pa + 63) / 64), dim3(64), 0, st, partial_ws, blocks, Pa, out,
                     loss_ws, (double*)nullptr);
  SPO_LAUNCH_CHECK("spo_cpo_fvp");
  return 0;
}

extern "C" int spo_cpo_linesearch_eval(const float* theta, const float* obs, const float* act, const float* logp_old,
                                       const float* adv_r, const float* adv_c, const float* mean_old,
                                       const float* log_std_old, int64_t rows, int obs_dim, int act_dim,
                                       double* partial_ws, int partial_capacity, double* sums3_out, void* stream) {
  if (int rc = check(obs_dim, act_dim)) return rc;
  SPO_REQUIRE(theta && obs && act && logp_old && adv_r && adv_c && mean_old && log_std_old && partial_ws && sums3_out &&
                  rows > 0, "cpo_linesearch_eval: bad args");
  int64_t blocks = (rows + 63) / 64;
  if (blocks > 1024) blocks = 1024;
  if (blocks * 3 > partial_capacity) blocks = partial_capacity / 3;
  SPO_REQUIRE(blocks >= 1, "cpo_linesearch_eval: partial capacity too small");
  LsArgs a{theta, obs, act, logp_old, adv_r, adv_c, mean_old, log_std_old, partial_ws, rows, obs_dim, act_dim};
  hipStream_t st = (hipStream_t)stream;
  switch (pick_kin(obs_dim)) {
    case 16: hipLaunchKernelGGL((cpo_linesearch_kernel<16>), dim3((unsigned)blocks), dim3(256), 0, st, a); break;
    case 32: hipLaunchKernelGGL((cpo_linesearch_kernel<32>), dim3((unsigned)blocks), dim3(256), 0, st, a); break;
    default: hipLaunchKernelGGL((cpo_linesearch_kernel<64>), dim3((unsigned)blocks), dim3(256), 0, st, a); break;
  }
  hipLaunchKernelGGL(sum3_kernel, dim3(1), dim3(64), 0, st, partial_ws, (int)blocks, sums3_out);
  SPO_LAUNCH_CHECK("spo_cpo_linesearch_eval");
  return 0;
}

// ---- obs_dim 65..128: the same three primitives on the KIN = 128 forms (see the head of this file)
extern "C" int spo_cpo128_supported(int obs_dim, int act_dim) {
  return (obs_dim >= 65 && obs_dim <= 128 && act_dim >= 1 && act_dim <= SPO_MAX_ACT) ? 1 : 0;
}

extern "C" int spo_cpo128_num_partials(int64_t rows) { return spo_cpo_num_partials(rows); }

extern "C" int spo_cpo128_surrogate_grad(const float* theta, const float* obs, const float* act, const float* logp_old,
                                         const float* adv, float sign, int64_t rows, int obs_dim, int act_dim,
                                         float* partial_ws, double* loss_ws, float* grad_out, double* loss_sum_out,
                                         void* stream) {
  if (int rc = check128(obs_dim, act_dim)) return rc;
  SPO_REQUIRE(theta && obs && act && logp_old && adv && partial_ws && loss_ws && grad_out && loss_sum_out && rows > 0,
              "cpo128_surrogate_grad: bad args");
  const int blocks = spo_cpo128_num_partials(rows);
  CpoArgs a{theta, nullptr, obs, act, logp_old, adv, rows, obs_dim, act_dim, sign, partial_ws, loss_ws};
  hipStream_t st = (hipStream_t)stream;
  if (int rc = launch_cpo128<MODE_SURR>(a, blocks, st)) return rc;
  const int Pa = spo::actor_size(obs_dim, act_dim);
  hipLaunchKernelGGL(reduce_partials_kernel, dim3((Pa + 63) / 64), dim3(64), 0, st, partial_ws, blocks, Pa, grad_out,
                     loss_ws, loss_sum_out);
  SPO_LAUNCH_CHECK("spo_cpo128_surrogate_grad");
  return 0;
}

extern "C" int spo_cpo128_fvp(const float* theta, const float* obs, const float* vec, int64_t rows, int obs_dim,
                              int act_dim, float* partial_ws, double* loss_ws, float* out, void* stream) {
  if (int rc = check128(obs_dim, act_dim)) return rc;
  SPO_REQUIRE(theta && obs && vec && partial_ws && loss_ws && out && rows > 0, "cpo128_fvp: bad args");
  const int blocks = spo_cpo128_num_partials(rows);
  CpoArgs a{theta, vec, obs, nullptr, nullptr, nullptr, rows, obs_dim, act_dim, 1.f, partial_ws, loss_ws};
  hipStream_t st = (hipStream_t)stream;
  if (int rc = launch_cpo128<MODE_FVP_REUSE>(a, blocks, st)) return rc;
  const int Pa = spo::actor_size(obs_dim, act_dim);
  hipLaunchKernelGGL(reduce_partials_kernel, dim3((Pa + 63) / 64), dim3(64), 0, st, partial_ws, blocks, Pa, out,
                     loss_ws, (double*)nullptr);
  SPO_LAUNCH_CHECK("spo_cpo128_fvp");
  return 0;
}
extern "C" int spo_cpo128_linesearch_eval(const float* theta, const float* obs, const float* act, const float* logp_old,
                                          const float* adv_r, const float* adv_c, const float* mean_old,
                                          const float* log_std_old, int64_t rows, int obs_dim, int act_dim,
                                          double* partial_ws, int partial_capacity, double* sums3_out, void* stream) {
  if (int rc = check128(obs_dim, act_dim)) return rc;
  SPO_REQUIRE(theta && obs && act && logp_old && adv_r && adv_c && mean_old && log_std_old && partial_ws && sums3_out &&
                  rows > 0, "cpo128_linesearch_eval: bad args");
  int64_t blocks = (rows + 63) / 64;
  if (blocks > 1024) blocks = 1024;
  if (blocks * 3 > partial_capacity) blocks = partial_capacity / 3;
  SPO_REQUIRE(blocks >= 1, "cpo128_linesearch_eval: partial capacity too small");
  LsArgs a{theta, obs, act, logp_old, adv_r, adv_c, mean_old, log_std_old, partial_ws, rows, obs_dim, act_dim};
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL((cpo_linesearch_kernel<128>), dim3((unsigned)blocks), dim3(256), 0, st, a);
  hipLaunchKernelGGL(sum3_kernel, dim3(1), dim3(64), 0, st, partial_ws, (int)blocks, sums3_out);
  SPO_LAUNCH_CHECK("spo_cpo128_linesearch_eval");
  return 0;
}

// ---- obs_dim 129..512, act_dim 1..32 (HumanoidVelocity: 376 / 17): the spo_cpo512_* entry points.
// W1 (and the direction's V1) are not LDS-resident: every 64-row chunk streams them from global memory (L2) in 64-feature
// slices of 64 x 68 floats through the transposed buffers P / Q, which are idle during the forward pass.  The tail of the
// network (b1, W2, b2, W3 as two 16-row output tiles, b3) stays resident.  The backward pass runs the sub-phases of
// MODE_FVP_REUSE in both modes, with one dW1 sub-phase per slice of X^T; the observations are re-read per slice (they were
// read microseconds earlier) instead of being held in up to 128 registers next to the 128 dW1 accumulators.  Barrier rule of
// every (sub-)phase: one barrier before P / Q / R are written, one before they are read.
namespace {
using namespace spo;

constexpr int S_MAXS = 8;                  // 64-feature slices of W1 at obs_dim 512
constexpr int S_NO = 2;                    // 16-row output tiles: act_dim <= 32
constexpr int S_MAX_ACT = S_NO * OUTP;

struct TailLds {                           // the resident part of one network image: everything but W1
  static constexpr int B1 = 0;
  static constexpr int W2 = B1 + HID;
  static constexpr int B2 = W2 + HID * LDH;
  static constexpr int W3 = B2 + HID;
  static constexpr int B3 = W3 + S_MAX_ACT * LDH;
  static constexpr int SIZE = B3 + S_MAX_ACT;      // multiple of 4 floats
};

template <int MODE>
struct Cpo512Lds {
  static constexpr int W = 0;
  static constexpr int V = TailLds::SIZE;                                  // FVP only
  static constexpr int P = (MODE == MODE_SURR ? 1 : 2) * TailLds::SIZE;    // W1 slice, H1^T, H2^T, X^T slices
  static constexpr int Q = P + HID * LDB;                                  // V1 slice, dZ2^T, dZ1^T
  static constexpr int R = Q + HID * LDB;                                  // dO^T, 32 rows
  static constexpr int RED = R + S_MAX_ACT * LDB;
  static constexpr int SIZE = RED + 4 * S_MAX_ACT;
};

__device__ inline void stage_tail(const float* __restrict__ theta, const NetGeom g, float* lds, int tid) {
  using T = TailLds;
  for (int i = tid; i < T::SIZE / 4; i += 256) reinterpret_cast<f4*>(lds)[i] = f4{0.f, 0.f, 0.f, 0.f};
  __syncthreads();
  const int c0 = (tid & 15) * 4, r0 = tid >> 4;
  for (int r = r0; r < HID; r += 16) {
    const float* src = theta + g.w2() + r * HID + c0;
#pragma unroll
    for (int e = 0; e < 4; ++e) lds[T::W2 + r * LDH + c0 + e] = src[e];
  }
  for (int r = r0; r < g.OUT; r += 16) {
    const float* src = theta + g.w3() + r * HID + c0;
#pragma unroll
    for (int e = 0; e < 4; ++e) lds[T::W3 + r * LDH + c0 + e] = src[e];
  }
  for (int i = tid; i < HID; i += 256) { lds[T::B1 + i] = theta[g.b1() + i]; lds[T::B2 + i] = theta[g.b2() + i]; }
  for (int i = tid; i < g.OUT; i += 256) lds[T::B3 + i] = theta[g.b3() + i];
}

// This thread's sixteen elements of slice s of a row-major [64][D] matrix: rows (tid >> 4) + 16k, columns 64s + 4(tid & 15) .. + 3.
// Loads only, and unclamped: a ragged last slice reads at most 63 floats past its row, i.e. the next row or -- behind row 63 --
// the b1 and W2 blocks that follow W1 in both flat layouts (index < 64 D + 64).  The columns at and beyond D are zeroed when the
// slice is stored, one step later.
__device__ __forceinline__ void load_w1_slice_raw(const float* __restrict__ W, int D, int s, int tid, f4 (&w)[4]) {
  const int c0 = 64 * s + 4 * (tid & 15), r0 = tid >> 4;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float* src = W + (r0 + 16 * k) * D + c0;
#pragma unroll
    for (int e = 0; e < 4; ++e) w[k][e] = src[e];
  }
}
__device__ __forceinline__ void store_w1_slice(float* buf, int D, int s, int tid, const f4 (&w)[4]) {
  const int cl = 4 * (tid & 15), c0 = 64 * s + cl, r0 = tid >> 4;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    f4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = c0 + e < D ? w[k][e] : 0.f;
    *reinterpret_cast<f4*>(buf + (r0 + 16 * k) * LDB + cl) = v;
  }
}
// B-operand tiles of slice s of one observation row: x[nt][reg] = obs[64s + 16nt + 4q + reg]; loads, then the mask.  The row is
// given as the chunk's (uniform) base and this lane's 32-bit element offset into the chunk (< 64 * 512): one address register per
// load instead of two.  (X4: obs_dim is a multiple of 4, so a row's tiles are aligned 16-byte loads)
template <bool X4>
__device__ __forceinline__ void load_obs_slice_raw(const float* __restrict__ chunk, unsigned rowoff, int D, int s, int q,
                                                   f4 (&x)[4]) {
  if (X4) {
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int c = 64 * s + 16 * nt + 4 * q;
      x[nt] = *reinterpret_cast<const f4*>(chunk + (rowoff + (unsigned)(c < D ? c : 0)));
    }
  } else {
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = 64 * s + 16 * nt + 4 * q + e;
        x[nt][e] = chunk[rowoff + (unsigned)(c < D ? c : 0)];
      }
  }
}
__device__ __forceinline__ void mask_obs_slice(int D, int s, int q, f4 (&x)[4]) {
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int e = 0; e < 4; ++e) x[nt][e] = (64 * s + 16 * nt + 4 * q + e) < D ? x[nt][e] : 0.f;
}

// Forward of one network for the 16 batch columns of a wave, layer 1 accumulated over ns streamed slices (ascending features:
// the order of layer_hidden).  The WHOLE workgroup calls this together (barriers).  TAN: the tangent's layer 1 (V1 x + vb1)
// rides along through Q.  The three kernels below share it, so the line search reproduces the snapshot's means bit for bit.
template <bool TAN, bool X4>
__device__ __forceinline__ void forward512(const float* Wl, const float* Vl, const float* __restrict__ W1g,
                                           const float* __restrict__ V1g, const float* __restrict__ xchunk, unsigned xoff, int D, int ns,
                                           bool two, float* P, float* Q, int tid, int j, int q, f4 (&h1)[4], f4 (&h2)[4],
                                           f4 (&o)[S_NO], f4 (&t1)[4]) {
  using T = TailLds;
  f4 acc[4], wr[4], vr[4], xr[4];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) acc[mt] = *reinterpret_cast<const f4*>(Wl + T::B1 + 16 * mt + 4 * q);
  if (TAN) {
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) t1[mt] = *reinterpret_cast<const f4*>(Vl + T::B1 + 16 * mt + 4 * q);
  }
  load_w1_slice_raw(W1g, D, 0, tid, wr);
  if (TAN) load_w1_slice_raw(V1g, D, 0, tid, vr);
  load_obs_slice_raw<X4>(xchunk, xoff, D, 0, q, xr);
#pragma unroll 1
  for (int s = 0; s < ns; ++s) {
    __syncthreads();
    store_w1_slice(P, D, s, tid, wr);
    if (TAN) store_w1_slice(Q, D, s, tid, vr);
    f4 xs[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) xs[nt] = xr[nt];
    mask_obs_slice(D, s, q, xs);
    if (s + 1 < ns) {                       // the next slice's loads fly under this slice's products
      load_w1_slice_raw(W1g, D, s + 1, tid, wr);
      if (TAN) load_w1_slice_raw(V1g, D, s + 1, tid, vr);
      load_obs_slice_raw<X4>(xchunk, xoff, D, s + 1, q, xr);
    }
    __syncthreads();
    layer_accum<4>(P, LDB, xs, acc, j, q);
    if (TAN) layer_accum<4>(Q, LDB, xs, t1, j, q);
  }
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) h1[mt] = fast_tanh4(acc[mt]);
  layer_hidden<4, true>(Wl + T::W2, LDH, Wl + T::B2, h1, h2, j, q);
  o[0] = layer_out(Wl + T::W3, Wl + T::B3, h2, j, q);
  o[1] = f4{0.f, 0.f, 0.f, 0.f};
  if (two) o[1] = layer_out(Wl + T::W3 + OUTP * LDH, Wl + T::B3 + OUTP, h2, j, q);
}

template <int MODE, bool X4>
__global__ __launch_bounds__(256, 1) void cpo512_actor_kernel(CpoArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  using U = Cpo512Lds<MODE>;
  using T = TailLds;
  constexpr bool FVP = MODE != MODE_SURR;
  constexpr int P = U::P, Q = U::Q, R = U::R;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, q = lane >> 4;
  const int D = a.D, A = a.A;
  const int ns = (D + 63) >> 6;
  const bool two = A > OUTP;
  const NetGeom g = net_geom(D, A, 2);
  const int ls_off = g.off - A;
  const int Pa = actor_size(D, A);
  stage_tail(a.theta, g, lds + U::W, tid);
  NetGeom gv = g;
  gv.off = A;                                     // the direction uses the actor's own flat layout: W1 after its log_std block
  if (FVP) stage_tail(a.vec, gv, lds + U::V, tid);
  __syncthreads();
  const float* Wl = lds + U::W;
  const float* Vl = lds + U::V;
  const float* W1g = a.theta + g.w1();
  const float* V1g = FVP ? a.vec + gv.w1() : a.theta;
  float* const red = lds + U::RED;

  float ivar[S_NO][4], lsd[S_NO][4], amask[S_NO][4];
#pragma unroll
  for (int t = 0; t < S_NO; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ai = 16 * t + 4 * q + r;
      const bool on = ai < A;
      const float lsv = on ? a.theta[ls_off + ai] : 0.f;
      const float sdv = expf(lsv);
      amask[t][r] = on ? 1.f : 0.f;
      ivar[t][r] = 1.f / (sdv * sdv);
      lsd[t][r] = on ? lsv + LOG_SQRT_2PI : 0.f;
    }
  const int orow = 16 * wave + 4 * q;
  const int mycol = 16 * wave + j;
  f4 aW1[4 * S_MAXS], aW2[4], aW3[S_NO], dls[S_NO];
#pragma unroll
  for (int nt = 0; nt < 4 * S_MAXS; ++nt) aW1[nt] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) aW2[nt] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < S_NO; ++t) { aW3[t] = f4{0.f, 0.f, 0.f, 0.f}; dls[t] = f4{0.f, 0.f, 0.f, 0.f}; }
  float db1 = 0.f, db2 = 0.f, db3[S_NO] = {0.f, 0.f};
  double lsum = 0.0;
  const float inv_m = (float)(1.0 / (double)a.M);
  const float inv_ma = (float)(1.0 / ((double)a.M * (double)A));

  const int64_t nchunks = (a.M + 63) / 64;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int64_t row = c * 64 + mycol;
    const bool cv = row < a.M;
    const int64_t smp = cv ? row : a.M - 1;
    const float* xchunk = a.obs + c * 64 * D;                       // uniform; this lane's row as a 32-bit offset
    const unsigned xoff = (unsigned)(smp - c * 64) * (unsigned)D;
    f4 h1[4], h2[4], o[S_NO], t1[4];
    forward512<FVP, X4>(Wl, Vl, W1g, V1g, xchunk, xoff, D, ns, two, lds + P, lds + Q, tid, j, q, h1, h2, o, t1);
    f4 dO[S_NO];
    if (MODE == MODE_SURR) {
      float lp = 0.f, dif[S_NO][4];
#pragma unroll
      for (int t = 0; t < S_NO; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int ai = 16 * t + 4 * q + r;
          const float av = a.act[smp * A + (ai < A ? ai : 0)];
          dif[t][r] = (ai < A ? av : 0.f) - o[t][r];
          lp += -(dif[t][r] * dif[t][r]) * (0.5f * ivar[t][r]) - lsd[t][r];
        }
      lp += __shfl_xor(lp, 16);
      lp += __shfl_xor(lp, 32);
      const float ratio = expf(lp - a.logp_old[smp]);                 // cpo.py:358 / :374
      const float adv = a.adv[smp];
      if (q == 0 && cv) lsum += (double)(ratio * adv);
      const float dlp = cv ? a.sign * adv * ratio * inv_m : 0.f;      // d(sign*mean(ratio*adv))/dlogp
#pragma unroll
      for (int t = 0; t < S_NO; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float z = dif[t][r] * ivar[t][r];
          dO[t][r] = dlp * z;
          dls[t][r] = fmaf(dlp * amask[t][r], dif[t][r] * z - 1.f, dls[t][r]);
        }
    } else {
      // tangent pass behind layer 1 (forward512 left V1 x + vb1 in t1): as in cpo_actor_kernel
      f4 t2[4];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) t1[mt][r] *= fmaf(-h1[mt][r], h1[mt][r], 1.f);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) t2[mt] = *reinterpret_cast<const f4*>(Vl + T::B2 + 16 * mt + 4 * q);
      layer_accum<4>(Wl + T::W2, LDH, t1, t2, j, q);
      __builtin_amdgcn_sched_barrier(0);
      layer_accum<4>(Vl + T::W2, LDH, h1, t2, j, q);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) t2[mt][r] *= fmaf(-h2[mt][r], h2[mt][r], 1.f);
      const float cm = cv ? inv_ma : 0.f;
#pragma unroll
      for (int t = 0; t < S_NO; ++t) {
        dO[t] = f4{0.f, 0.f, 0.f, 0.f};
        if (t == 0 || two) {
          f4 mud = *reinterpret_cast<const f4*>(Vl + T::B3 + 16 * t + 4 * q);
          mud = out_accum(Wl + T::W3 + 16 * t * LDH, t2, mud, j, q);
          mud = out_accum(Vl + T::W3 + 16 * t * LDH, h2, mud, j, q);
#pragma unroll
          for (int r = 0; r < 4; ++r) dO[t][r] = mud[r] * ivar[t][r] * amask[t][r] * cm;
        }
      }
    }
    // the first X^T slice of the dW1 sub-phases: in flight under everything up to there
    f4 xr[4];
    load_obs_slice_raw<X4>(xchunk, xoff, D, 0, q, xr);

    // ---- backward through the MLP
    f4 dz2[4], dz1[4];
    {
      f4 acc[4];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) acc[mt] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < S_NO; ++t)
        if (t == 0 || two) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
              acc[mt] = mfma4(Wl[T::W3 + (16 * t + 4 * q + r) * LDH + 16 * mt + j], dO[t][r], acc[mt]);
        }
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) dz2[mt][r] = acc[mt][r] * fmaf(-h2[mt][r], h2[mt][r], 1.f);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) acc[mt] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int mt = 0; mt < 4; ++mt)
            acc[mt] = mfma4(Wl[T::W2 + (16 * nt + 4 * q + r) * LDH + 16 * mt + j], dz2[nt][r], acc[mt]);
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) dz1[mt][r] = acc[mt][r] * fmaf(-h1[mt][r], h1[mt][r], 1.f);
    }

    // 1: P = H1^T, Q = dZ2^T, R = dO^T  ->  dW2, db2
    __syncthreads();
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = (16 * mt + 4 * q + r) * LDB + mycol;
        lds[P + f] = h1[mt][r];
        lds[Q + f] = dz2[mt][r];
      }
#pragma unroll
    for (int t = 0; t < S_NO; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) lds[R + (16 * t + 4 * q + r) * LDB + mycol] = dO[t][r];
    __syncthreads();
    {
      f4 az[4];
      float rs = 0.f;
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        az[r4] = *reinterpret_cast<const f4*>(lds + Q + (16 * wave + j) * LDB + 16 * r4 + 4 * q);
        rs += (az[r4][0] + az[r4][1]) + (az[r4][2] + az[r4][3]);
      }
      db2 += rs;
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        f4 bh[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
          bh[nt] = *reinterpret_cast<const f4*>(lds + P + (16 * nt + j) * LDB + 16 * r4 + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) aW2[nt] = mfma4(az[r4][e], bh[nt][e], aW2[nt]);
      }
    }
    // 2: P = H2^T, Q = dZ1^T  ->  dW3 (both output tiles), db3; this wave's dZ1^T rows go to registers, db1
    __syncthreads();
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = (16 * mt + 4 * q + r) * LDB + mycol;
        lds[P + f] = h2[mt][r];
        lds[Q + f] = dz1[mt][r];
      }
    __syncthreads();
    f4 az1[4];
    {
#pragma unroll
      for (int t = 0; t < S_NO; ++t)
        if (t == 0 || two) {
          float rs = 0.f;
#pragma unroll
          for (int r4 = 0; r4 < 4; ++r4) {
            const f4 az = *reinterpret_cast<const f4*>(lds + R + (16 * t + j) * LDB + 16 * r4 + 4 * q);
            rs += (az[0] + az[1]) + (az[2] + az[3]);
            const f4 bh = *reinterpret_cast<const f4*>(lds + P + (16 * wave + j) * LDB + 16 * r4 + 4 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e) aW3[t] = mfma4(az[e], bh[e], aW3[t]);
          }
          db3[t] += rs;
        }
      float rs = 0.f;
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        az1[r4] = *reinterpret_cast<const f4*>(lds + Q + (16 * wave + j) * LDB + 16 * r4 + 4 * q);
        rs += (az1[r4][0] + az1[r4][1]) + (az1[r4][2] + az1[r4][3]);
      }
      db1 += rs;
    }
    // 3 ..: P = X^T features 64s .. 64s + 63  ->  dW1 columns of slice s
#pragma unroll
    for (int s = 0; s < S_MAXS; ++s) {
      if (s < ns) {
        __syncthreads();
        mask_obs_slice(D, s, q, xr);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int e = 0; e < 4; ++e) lds[P + (16 * nt + 4 * q + e) * LDB + mycol] = xr[nt][e];
        if (s + 1 < ns) load_obs_slice_raw<X4>(xchunk, xoff, D, s + 1, q, xr);
        __syncthreads();
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          f4 bh[4];
#pragma unroll
          for (int nt = 0; nt < 4; ++nt)
            bh[nt] = *reinterpret_cast<const f4*>(lds + P + (16 * nt + j) * LDB + 16 * r4 + 4 * q);
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) aW1[4 * s + nt] = mfma4(az1[r4][e], bh[nt][e], aW1[4 * s + nt]);
        }
      }
    }
  }

  // ---- emit this workgroup's partial flat vector (actor layout) -- every element written exactly once
  db1 += __shfl_xor(db1, 16); db1 += __shfl_xor(db1, 32);
  db2 += __shfl_xor(db2, 16); db2 += __shfl_xor(db2, 32);
#pragma unroll
  for (int t = 0; t < S_NO; ++t) { db3[t] += __shfl_xor(db3[t], 16); db3[t] += __shfl_xor(db3[t], 32); }
#pragma unroll
  for (int t = 0; t < S_NO; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v = dls[t][r];
      v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); v += __shfl_xor(v, 8);
      if (j == 0) red[wave * S_MAX_ACT + 16 * t + 4 * q + r] = v;      // [wave][32]
    }
  const double lw = wave_sum_d(lsum);
  __shared__ double lred[4];
  if (lane == 0) lred[wave] = lw;
  __syncthreads();
  float* out = a.partial + (int64_t)blockIdx.x * Pa;
  const int w1 = A, b1 = w1 + HID * D, w2 = b1 + HID, b2 = w2 + HID * HID, w3 = b2 + HID, b3 = w3 + A * HID;
#pragma unroll
  for (int nt = 0; nt < 4 * S_MAXS; ++nt)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (16 * nt + j < D) out[w1 + (orow + r) * D + 16 * nt + j] = aW1[nt][r];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int r = 0; r < 4; ++r) out[w2 + (orow + r) * HID + 16 * nt + j] = aW2[nt][r];
#pragma unroll
  for (int t = 0; t < S_NO; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (16 * t + 4 * q + r < A) out[w3 + (16 * t + 4 * q + r) * HID + 16 * wave + j] = aW3[t][r];
  if (q == 0) { out[b1 + 16 * wave + j] = db1; out[b2 + 16 * wave + j] = db2; }
#pragma unroll
  for (int t = 0; t < S_NO; ++t)
    if (wave == 0 && q == 0 && 16 * t + j < A) out[b3 + 16 * t + j] = db3[t];
  if (wave == 0 && j == 0) {
#pragma unroll
    for (int t = 0; t < S_NO; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ai = 16 * t + 4 * q + r;
        if (ai < A)
          out[ai] = (red[ai] + red[S_MAX_ACT + ai]) + (red[2 * S_MAX_ACT + ai] + red[3 * S_MAX_ACT + ai]);
      }
  }
  if (tid == 0) a.partial_loss[blockIdx.x] = (lred[0] + lred[1]) + (lred[2] + lred[3]);
}

// Line-search sums (cpo.py:473-491) and the snapshot's means (cpo.py:361: old_distribution) on forward512.  MEAN_ONLY: the
// means go to mean_out and LsArgs::theta / obs / M / D / A are the only fields read.
template <bool MEAN_ONLY, bool X4>
__global__ __launch_bounds__(256) void cpo512_forward_kernel(LsArgs a, float* mean_out) {
  __shared__ __attribute__((aligned(16))) float lds[TailLds::SIZE + HID * LDB];
  __shared__ double red[4][3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, q = lane >> 4;
  const int D = a.D, A = a.A;
  const int ns = (D + 63) >> 6;
  const bool two = A > OUTP;
  const NetGeom g = net_geom(D, A, 2);
  stage_tail(a.theta, g, lds, tid);
  __syncthreads();
  float* const P = lds + TailLds::SIZE;
  const float* W1g = a.theta + g.w1();
  const int ls_off = g.off - A;
  float ivar[S_NO][4], lsd[S_NO][4], sdn[S_NO][4], sdo[S_NO][4];
  if (!MEAN_ONLY) {
#pragma unroll
    for (int t = 0; t < S_NO; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ai = 16 * t + 4 * q + r;
        const bool on = ai < A;
        const float lsv = on ? a.theta[ls_off + ai] : 0.f;
        sdn[t][r] = expf(lsv);
        sdo[t][r] = on ? expf(a.log_std_old[ai]) : 1.f;
        ivar[t][r] = 1.f / (sdn[t][r] * sdn[t][r]);
        lsd[t][r] = on ? logf(sdn[t][r]) + LOG_SQRT_2PI : 0.f;
      }
  }
  double s_r = 0, s_c = 0, s_kl = 0;
  const int64_t nchunks = (a.M + 63) / 64;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int64_t row = c * 64 + 16 * wave + j;
    const bool valid = row < a.M;
    const int64_t rr = valid ? row : a.M - 1;
    f4 h1[4], h2[4], mu[S_NO], unused[4];
    forward512<false, X4>(lds, lds, W1g, W1g, a.obs + c * 64 * D, (unsigned)(rr - c * 64) * (unsigned)D, D, ns, two, P, P, tid, j, q, h1, h2, mu, unused);
    if (MEAN_ONLY) {
#pragma unroll
      for (int t = 0; t < S_NO; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int ai = 16 * t + 4 * q + r;
          if (valid && ai < A) mean_out[rr * A + ai] = mu[t][r];
        }
      continue;
    }
    float lp = 0.f, kl = 0.f;
#pragma unroll
    for (int t = 0; t < S_NO; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ai = 16 * t + 4 * q + r;
        if (ai < A) {
          const float dif = a.act[rr * A + ai] - mu[t][r];
          lp += -(dif * dif) * (0.5f * ivar[t][r]) - lsd[t][r];
          const float ratio = sdo[t][r] / sdn[t][r];
          const float vr = ratio * ratio;
          const float dm = (a.mean_old[rr * A + ai] - mu[t][r]) / sdn[t][r];
          kl += 0.5f * (vr + dm * dm - 1.f - logf(vr));
        }
      }
    lp += __shfl_xor(lp, 16); lp += __shfl_xor(lp, 32);
    const float ratio = expf(lp - a.logp_old[rr]);
    if (valid) {
      s_kl += (double)kl;                       // every lane holds its own dims
      if (q == 0) { s_r += (double)(ratio * a.adv_r[rr]); s_c += (double)(ratio * a.adv_c[rr]); }
    }
  }
  if (MEAN_ONLY) return;
  s_r = wave_sum_d(s_r); s_c = wave_sum_d(s_c); s_kl = wave_sum_d(s_kl);
  if (lane == 0) { red[wave][0] = s_r; red[wave][1] = s_c; red[wave][2] = s_kl; }
  __syncthreads();
  if (tid < 3) a.partials[blockIdx.x * 3 + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

template <int MODE, bool X4>
int launch_cpo512_form(const CpoArgs& a, int blocks, hipStream_t st) {
  constexpr size_t sh = Cpo512Lds<MODE>::SIZE * sizeof(float);
  static_assert(sh <= 160 * 1024, "cpo512: LDS form does not fit one workgroup");
  static bool attr_done[spo::SPO_MAX_DEVICES] = {};
  return spo::launch_dyn_lds(&cpo512_actor_kernel<MODE, X4>, attr_done, "cpo512", dim3(blocks), dim3(256), sh, st, a);
}
template <int MODE>
int launch_cpo512(const CpoArgs& a, int blocks, hipStream_t st) {
  return (a.D & 3) == 0 ? launch_cpo512_form<MODE, true>(a, blocks, st) : launch_cpo512_form<MODE, false>(a, blocks, st);
}

template <bool MEAN_ONLY>
void launch_forward512(const LsArgs& a, float* mean_out, unsigned blocks, hipStream_t st) {
  if ((a.D & 3) == 0) hipLaunchKernelGGL((cpo512_forward_kernel<MEAN_ONLY, true>), dim3(blocks), dim3(256), 0, st, a, mean_out);
  else hipLaunchKernelGGL((cpo512_forward_kernel<MEAN_ONLY, false>), dim3(blocks), dim3(256), 0, st, a, mean_out);
}

int check512(int D, int A) {
  if (D < 129 || D > 512) return spo::fail(-2, "cpo512: obs_dim %d outside [129,512]", D);
  if (A < 1 || A > S_MAX_ACT) return spo::fail(-2, "cpo512: act_dim %d outside [1,32]", A);
  return 0;
}

}  // namespace

extern "C" int spo_cpo512_supported(int obs_dim, int act_dim) {
  return (obs_dim >= 129 && obs_dim <= 512 && act_dim >= 1 && act_dim <= S_MAX_ACT) ? 1 : 0;
}

extern "C" int spo_cpo512_num_partials(int64_t rows) { return spo_cpo_num_partials(rows); }

// cpo.py:356-365, :372-381
extern "C" int spo_cpo512_surrogate_grad(const float* theta, const float* obs, const float* act, const float* logp_old,
                                         const float* adv, float sign, int64_t rows, int obs_dim, int act_dim,
                                         float* partial_ws, double* loss_ws, float* grad_out, double* loss_sum_out,
                                         void* stream) {
  if (int rc = check512(obs_dim, act_dim)) return rc;
  SPO_REQUIRE(theta && obs && act && logp_old && adv && partial_ws && loss_ws && grad_out && loss_sum_out && rows > 0,
              "cpo512_surrogate_grad: bad args");
  const int blocks = spo_cpo512_num_partials(rows);
  CpoArgs a{theta, nullptr, obs, act, logp_old, adv, rows, obs_dim, act_dim, sign, partial_ws, loss_ws};
  hipStream_t st = (hipStream_t)stream;
  if (int rc = launch_cpo512<MODE_SURR>(a, blocks, st)) return rc;
  const int Pa = spo::actor_size(obs_dim, act_dim);
  hipLaunchKernelGGL(reduce_partials_kernel, dim3((Pa + 63) / 64), dim3(64), 0, st, partial_ws, blocks, Pa, grad_out,
                     loss_ws, loss_sum_out);
  SPO_LAUNCH_CHECK("spo_cpo512_surrogate_grad");
  return 0;
}

// cpo.py:132-157
extern "C" int spo_cpo512_fvp(const float* theta, const float* obs, const float* vec, int64_t rows, int obs_dim,
                              int act_dim, float* partial_ws, double* loss_ws, float* out, void* stream) {
  if (int rc = check512(obs_dim, act_dim)) return rc;
  SPO_REQUIRE(theta && obs && vec && partial_ws && loss_ws && out && rows > 0, "cpo512_fvp: bad args");
  const int blocks = spo_cpo512_num_partials(rows);
  CpoArgs a{theta, vec, obs, nullptr, nullptr, nullptr, rows, obs_dim, act_dim, 1.f, partial_ws, loss_ws};
  hipStream_t st = (hipStream_t)stream;
  if (int rc = launch_cpo512<MODE_FVP>(a, blocks, st)) return rc;
  const int Pa = spo::actor_size(obs_dim, act_dim);
  hipLaunchKernelGGL(reduce_partials_kernel, dim3((Pa + 63) / 64), dim3(64), 0, st, partial_ws, blocks, Pa, out,
                     loss_ws, (double*)nullptr);
  SPO_LAUNCH_CHECK("spo_cpo512_fvp");
  return 0;
}

// cpo.py:473-491
extern "C" int spo_cpo512_linesearch_eval(const float* theta, const float* obs, const float* act, const float* logp_old,
                                          const float* adv_r, const float* adv_c, const float* mean_old,
                                          const float* log_std_old, int64_t rows, int obs_dim, int act_dim,
                                          double* partial_ws, int partial_capacity, double* sums3_out, void* stream) {
  if (int rc = check512(obs_dim, act_dim)) return rc;
  SPO_REQUIRE(theta && obs && act && logp_old && adv_r && adv_c && mean_old && log_std_old && partial_ws && sums3_out &&
                  rows > 0, "cpo512_linesearch_eval: bad args");
  int64_t blocks = (rows + 63) / 64;
  if (blocks > 1024) blocks = 1024;
  if (blocks * 3 > partial_capacity) blocks = partial_capacity / 3;
  SPO_REQUIRE(blocks >= 1, "cpo512_linesearch_eval: partial capacity too small");
  LsArgs a{theta, obs, act, logp_old, adv_r, adv_c, mean_old, log_std_old, partial_ws, rows, obs_dim, act_dim};
  hipStream_t st = (hipStream_t)stream;
  launch_forward512<false>(a, nullptr, (unsigned)blocks, st);
  hipLaunchKernelGGL(sum3_kernel, dim3(1), dim3(64), 0, st, partial_ws, (int)blocks, sums3_out);
  SPO_LAUNCH_CHECK("spo_cpo512_linesearch_eval");
  return 0;
}

// cpo.py:361 (old_distribution = policy.actor(data["obs"])): the means, by the forward the line search runs
extern "C" int spo_cpo512_actor_mean(const float* theta, const float* obs, float* mean_out, int64_t rows, int obs_dim,
                                     int act_dim, void* stream) {
  if (int rc = check512(obs_dim, act_dim)) return rc;
  SPO_REQUIRE(theta && obs && mean_out && rows > 0, "cpo512_actor_mean: bad args");
  int64_t blocks = (rows + 63) / 64;
  if (blocks > 1024) blocks = 1024;
  LsArgs a{theta, obs, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, rows, obs_dim, act_dim};
  launch_forward512<true>(a, mean_out, (unsigned)blocks, (hipStream_t)stream);
  SPO_LAUNCH_CHECK("spo_cpo512_actor_mean");
  return 0;
}
