// Stand-alone check of csrc/adam_host.h (built and run by tests/test_wide_kernel_cases_host.py with the host compiler: the header
// makes no HIP call and includes no HIP header).  Prints one "ok <property>" line per property that holds, "FAIL <property>: <why>"
// otherwise, and "done <failures>" last; exits 1 when anything failed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include "adam_host.h"

namespace {

int g_failures = 0;
void report(const char* what, bool ok, const char* why = "") {
  if (ok) printf("ok %s\n", what);
  else { printf("FAIL %s: %s\n", what, why); ++g_failures; }
}
float from_bits(uint32_t u) { float f; memcpy(&f, &u, sizeof f); return f; }
uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, sizeof u); return u; }

}  // namespace

int main() {
  // ---- the betas configurations use: the weight is (float)(1.0 - beta) of the DECIMAL, not 1.f - (float)beta
  {
    const double named[] = {0.9, 0.999, 0.99, 0.95, 0.5, 0.0};
    bool meant = true, weight = true;
    for (double d : named) {
      double back = -1.0;
      float w = -1.f;
      meant = meant && spo::adam_beta_meant((float)d, &back) && back == d;
      weight = weight && spo::adam_one_minus_beta((float)d, &w) && bits_of(w) == bits_of((float)(1.0 - d));
      printf("beta %.3f: meant %.17g  weight %.9g  (1.f - beta: %.9g)\n", d, back, (double)w, (double)(1.f - (float)d));
    }
    report("named betas give back their decimal", meant);
    report("named betas give (float)(1.0 - beta)", weight);
    float w2 = 0.f;
    spo::adam_one_minus_beta(0.999f, &w2);
    report("the weight of 0.999 differs from 1.f - 0.999f", bits_of(w2) != bits_of(1.f - 0.999f) && std::fabs((double)w2 / 1e-3 - 1.0) < 1e-7);
  }
  // ---- every sampled float32 in [0, 1) round-trips bit for bit (a stride over the bit patterns, plus the ends and the denormals)
  {
    bool ok = true;
    uint64_t n = 0;
    const uint32_t one = bits_of(1.f);
    for (uint32_t u = 0; u < one; u += 7919) {
      double d;
      ok = ok && spo::adam_beta_meant(from_bits(u), &d) && bits_of((float)d) == u;
      ++n;
    }
    const uint32_t ends[] = {0u, 1u, 2u, 0x007fffffu, 0x00800000u, one - 1, one - 2, bits_of(0.1f), bits_of(0.3f), bits_of(1e-30f)};
    for (uint32_t u : ends) {
      double d;
      ok = ok && spo::adam_beta_meant(from_bits(u), &d) && bits_of((float)d) == u;
      ++n;
    }
    printf("round trip: %llu floats\n", (unsigned long long)n);
    report("sampled floats round-trip bit for bit", ok && n > 100000);
  }
  // ---- the per-thread memo gives what a fresh evaluation gives, in any order of asking
  {
    const float seq[] = {0.9f, 0.999f, 0.9f, 0.5f, 0.999f, 0.99f, 0.9f, 0.f, 0.f, 0.999f};
    bool ok = true;
    for (float b : seq) {
      float w;
      double d;
      double meant = -1.0;
      float w2 = -1.f;
      ok = ok && spo::adam_one_minus_beta(b, &w) && spo::adam_beta_meant(b, &d) && bits_of(w) == bits_of((float)(1.0 - d));
      ok = ok && spo::adam_beta_host(b, &meant, &w2) && meant == d && bits_of(w2) == bits_of(w);      // clocks and weights from one number
    }
    report("remembered weights equal fresh ones", ok);
  }
  // ---- no Adam has a beta outside [0, 1)
  {
    const float bad[] = {1.f, 1.5f, -0.1f, -0.f - 1e-30f, std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(),
                         std::numeric_limits<float>::quiet_NaN()};
    bool ok = true;
    for (float b : bad) {
      double d = 123.0;
      float w = 123.f;
      ok = ok && !spo::adam_beta_meant(b, &d) && !spo::adam_one_minus_beta(b, &w) && d == 123.0 && w == 123.f;
    }
    report("betas outside [0, 1) are refused", ok);
  }
  printf("done %d\n", g_failures);
  return g_failures ? 1 : 0;
}
