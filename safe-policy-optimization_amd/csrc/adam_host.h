// Host side of the wide-network path's Adam weights (no HIP include: tests/adam_host_check.cpp builds it with the host compiler).
//
// spo_ppo_cfg carries the betas as float32.  torch.optim.Adam holds them as Python floats and forms the two weights of the moment
// updates, 1 - beta1 and 1 - beta2, in double; the float32 kernels of torch then see float(1 - 0.999) = 1.00000005e-3.  Formed
// from the float32 beta, 1.f - 0.999f = 0.99998713e-3: 1.3e-5 relative off in every second moment, ten times what the float64
// yardstick allows (tests/wide_kernel_cases.py).  So the double the caller meant is recovered here -- the shortest decimal that
// rounds to the given float32, which is what Python prints for a float32 -- and 1 - beta is formed in double and rounded once.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace spo {

// The double whose shortest decimal form rounds to `b` in float32 (0.9f -> 0.9, 0.999f -> 0.999); (float)result == b always.
// false: b is outside [0, 1) or not a number -- no Adam has such a beta.
inline bool adam_beta_meant(float b, double* out) {
  if (!(b >= 0.f && b < 1.f)) return false;
  for (int digits = 1; digits <= 9; ++digits) {           // nine significant digits identify every float32
    char buf[40];
    snprintf(buf, sizeof buf, "%.*e", digits - 1, (double)b);
    const double d = strtod(buf, nullptr);
    if ((float)d == b) { *out = d; return true; }
  }
  *out = (double)b;                                        // (not reached for a finite float32)
  return true;
}

// Both host-side forms of one beta: *meant = the double the caller meant (the optimiser clocks beta^t are powers of THIS number,
// as torch's bias corrections are -- with the clocks on the float32 beta and the weight below on the decimal, a fresh optimiser's
// v / (1 - beta2^t) would be 1.3e-5 off at t = 1, where the two errors used to cancel) and *one_minus = (float)(1.0 - meant).  The
// last two betas asked for are remembered per thread: a training run asks for the same two at every step.
inline bool adam_beta_host(float b, double* meant, float* one_minus) {
  static thread_local uint32_t key[2] = {0xffffffffu, 0xffffffffu};   // (a NaN pattern: never a valid beta)
  static thread_local double dval[2] = {0.0, 0.0};
  static thread_local int next = 0;
  uint32_t bits;
  memcpy(&bits, &b, sizeof bits);
  double d = 0.0;
  bool hit = false;
  for (int k = 0; k < 2 && !hit; ++k)
    if (key[k] == bits) { d = dval[k]; hit = true; }
  if (!hit) {
    if (!adam_beta_meant(b, &d)) return false;
    key[next] = bits; dval[next] = d; next ^= 1;
  }
  *meant = d;
  *one_minus = (float)(1.0 - d);
  return true;
}
inline bool adam_one_minus_beta(float b, float* w) {
  double d;
  float v;
  if (!adam_beta_host(b, &d, &v)) return false;
  *w = v;
  return true;
}

}  // namespace spo
