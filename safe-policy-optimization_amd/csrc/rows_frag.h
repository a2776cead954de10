// Fragment loads and the row-band product shared by the 32-row-chunk kernels (cpo_rows.hip, ma_fvp.hip), gfx950.
// A chunk's activations are ROW images [32][132] in LDS; weights are read as v_mfma_f32_16x16x4_f32 A fragments straight from
// global memory (L2-resident), one fragment feeding both 16-row tiles of the chunk.
#pragma once
#include "mlp_mfma.h"

namespace spo {
namespace rows {

constexpr int ROWS = 32;                   // rows per chunk: two 16-row MFMA tiles
constexpr int NTHR = 256;                 // 4 waves, one per SIMD: 512 registers each
constexpr int VW = 2;                      // every wave plays two of the eight tile owners ("virtual waves" w and w + 4)
constexpr int MAXT = 8;                    // 16-wide tiles per layer dimension: widths and obs_dim up to 128
constexpr int MAXW = 16 * MAXT;
constexpr int MAXA = 16;
constexpr int LDI = MAXW + 4;
constexpr int LDO = MAXA + 4;
constexpr int IMG = ROWS * LDI;
constexpr int MAX_GRID = 256;              // one workgroup per CU

struct __attribute__((packed, aligned(4))) F4U { float v[4]; };      // a row fragment: the flat vector is only 4-byte aligned

// W[row][c0 .. c0 + 3], zero outside [nrows, ncols]; addresses clamped, never predicated.  Offsets are unsigned 32-bit values
// on a uniform base: one address register per load instead of a 64-bit pair.
__device__ __forceinline__ f4 ld_row4(const float* __restrict__ W, int ld, int row, int nrows, int c0, int ncols) {
  const bool rok = row < nrows;
  const unsigned base = (unsigned)((rok ? row : 0) * ld);
  f4 v;
  if ((ncols & 3) == 0) {
    const bool ok = rok && c0 < ncols;
    const F4U t = *reinterpret_cast<const F4U*>(&W[base + (unsigned)(c0 < ncols ? c0 : 0)]);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = ok ? t.v[e] : 0.f;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = c0 + e;
      const float t = W[base + (unsigned)(c < ncols ? c : 0)];
      v[e] = (rok && c < ncols) ? t : 0.f;
    }
  }
  return v;
}

// W[r0 .. r0 + 3][col]
__device__ __forceinline__ f4 ld_col4(const float* __restrict__ W, int ld, int r0, int nrows, int col, int ncols) {
  const bool cok = col < ncols;
  const unsigned base = (unsigned)(cok ? col : 0);
  f4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int r = r0 + e;
    const float t = W[base + (unsigned)((r < nrows ? r : 0) * ld)];
    v[e] = (cok && r < nrows) ? t : 0.f;
  }
  return v;
}

// which tile of `ntiles` 16-feature tiles, and which row tiles of the chunk, a wave computes in a forward / dH sub-phase
struct Unit { int t, r0, nr; bool on; };
__device__ __forceinline__ Unit unit_of(int wave, int ntiles) {
  if (ntiles > 4) return Unit{wave, 0, 2, wave < ntiles};
  return Unit{wave >> 1, wave & 1, 1, (wave >> 1) < ntiles};
}

// acc[i] += W[16 t + j][:] . IN[row tile r0 + i][:]   (every fragment of the row band in flight before the first product)
__device__ __forceinline__ void mm_rows(const float* __restrict__ Wg, int out, int in, const float* IN, const Unit u, int j, int q,
                                        f4 (&acc)[2]) {
  const int nk = (in + 15) >> 4;
  f4 af[MAXT];
#pragma unroll
  for (int nt = 0; nt < MAXT; ++nt)
    if (nt < nk) af[nt] = ld_row4(Wg, in, 16 * u.t + j, out, 16 * nt + 4 * q, in);
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

// b[f0 .. f0 + 3], zero from `out` on
__device__ __forceinline__ f4 bias4(const float* __restrict__ b, int f0, int out) {
  f4 v;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float t = b[(unsigned)(f0 + r < out ? f0 + r : 0)];
    v[r] = f0 + r < out ? t : 0.f;
  }
  return v;
}

// ---- the backward side of the multi-agent chunk kernels (ma_fvp.hip, ma_trpo_grads.hip; sum8 also ma_ls_eval.hip)
__device__ __forceinline__ float elu_grad(float a) { return a > 0.f ? 1.f : a + 1.f; }      // ELU' = exp(z) = a + 1 for z <= 0

// dst[32][LDI] <- rows c * 32 .. of src[B][W]; zero beyond W and past the batch (all 128 columns are written)
__device__ __forceinline__ void load_image(float* dst, const float* __restrict__ src, int W, int64_t row0, int64_t B, bool vec, int tid) {
  const int c0 = 4 * (tid & 31);
#pragma unroll
  for (int hh = 0; hh < ROWS / 8; ++hh) {
    const int lrow = (tid >> 5) + 8 * hh;
    const int64_t grow = row0 + lrow;
    f4 v = {0.f, 0.f, 0.f, 0.f};
    if (grow < B && c0 < W) {
      const float* p = src + grow * W + c0;
      if (vec) {
        v = *reinterpret_cast<const f4*>(p);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (c0 + e < W) v[e] = p[e];
      }
    }
    *reinterpret_cast<f4*>(dst + lrow * LDI + c0) = v;
  }
}

// acc[i] += sum over the feature tiles nt of layer l of  W[16 nt + 4 q ..][16 t + j] . DZ[row tile r0 + i][16 nt + 4 q ..]
__device__ __forceinline__ void mm_cols(const float* __restrict__ Wg, int out, int in, const float* DZ, int ldz, const Unit u, int j,
                                        int q, f4 (&acc)[2]) {
  const int ntm = (out + 15) >> 4;
  f4 af[MAXT];
#pragma unroll
  for (int nt = 0; nt < MAXT; ++nt)
    if (nt < ntm) af[nt] = ld_col4(Wg, in, 16 * nt + 4 * q, out, 16 * u.t + j, in);
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
}

__device__ __forceinline__ float sum8(float v) {      // over the 8 lanes of a row, the same order in every lane
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  return v;
}

}  // namespace rows
}  // namespace spo
