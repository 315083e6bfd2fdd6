// pair_log_run_host_shim.cpp — the running product of edge_alignment_amd/csrc/ea_pair_log.h (pl_run_*: one logarithm for a
// whole run of Cauchy factors, what a lane of the pose-per-lane kernel does over its sub-run) on the CPU.
// tests/test_pair_log_run_host.py builds this under AddressSanitizer and UBSan -- the exponent arithmetic of the
// renormalisation is the UBSan target -- and runs it.
//
// Runs of n = 1, 2, 127, 128 factors s = 1 + x are multiplied up and logged once, and compared with the sum of logl of the same
// ROUNDED factors.  Bar: relative error <= 8 * 2^-53 (pl_log's documented ~2 ulp with margin), every result finite, exactly 0
// where every factor is 1; the renormalisation never fires for factors near 1 and does fire in the cases built to need it.
// The pairwise sum the kernel used before (pl_log_pair per two factors) is measured beside it, as a figure only.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ea_pair_log.h"

namespace {

struct HostOps {
  static double frexp_mant(double x) { int e; return std::frexp(x, &e); }
  static int frexp_exp(double x) { int e; (void)std::frexp(x, &e); return e; }
  static double ldexp(double x, int e) { return std::ldexp(x, e); }
  // the device's reciprocal approximation is good to a few 1e-8 or better: a single-precision quotient stands in for it
  // (beyond float's range, where the quotient would be 0 or inf, the exponent is taken out first)
  static double rcp(double x) {
    int e;
    const double m = std::frexp(x, &e);
    return std::ldexp((double)(1.0f / (float)m), -e);
  }
  static double sconst(double c) { return c; }
};

// xorshift64*: the sweep is the same everywhere
uint64_t g_state = 0x9E3779B97F4A7C15ull;
double uniform01() {
  g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
  return (double)((g_state * 0x2545F4914F6CDD1Dull) >> 11) * (1.0 / 9007199254740992.0);
}
double log_uniform(double lo10, double hi10) { return std::pow(10.0, lo10 + (hi10 - lo10) * uniform01()); }

enum Case { kOnes, kBelowUlp, kTiny, kWide, kHuge, kOne1e200, kOne1e300, kCases };
const char *const kNames[kCases] = {"all ones", "x <= 1e-15", "x in [0, 1e-12]", "x = 10^U(-15, 8)", "x = 10^U(0, 100)",
                                    "one 1e200 among tiny x", "one factor at 1e300"};

void fill(Case c, std::vector<double> &s) {
  const size_t n = s.size(), special = (size_t)(uniform01() * n) % n;
  for (size_t i = 0; i < n; ++i) {
    double x = 0;
    switch (c) {
      case kOnes: x = 0; break;
      case kBelowUlp: x = 1e-15 * uniform01(); break;
      case kTiny: x = 1e-12 * uniform01(); break;
      case kWide: x = log_uniform(-15, 8); break;
      case kHuge: x = log_uniform(0, 100); break;
      case kOne1e200: x = i == special ? 1e200 : 1e-12 * uniform01(); break;
      case kOne1e300: x = i == special ? 1e300 : log_uniform(-15, 8); break;
      default: break;
    }
    s[i] = 1.0 + x;
  }
}

struct Stat { long double worst_run = 0, worst_pairs = 0; long renorms = 0, runs = 0; int worst_n = 0; };

bool measure(Case c, const std::vector<double> &s, Stat &st) {
  const int n = (int)s.size();
  long double ref = 0;
  for (double v : s) ref += logl((long double)v);
  double P = 1.0, L = 0.0;
  int E = 0;
  long renorms = 0;
  for (double v : s) renorms += ea::pl_run_step<HostOps>(P, L, E, v) ? 1 : 0;
  const double got = ea::pl_run_log<HostOps>(P, L, E);
  double pairs = 0;  // the form this replaces: one pl_log_pair per two factors, an odd run ends on a factor of 1
  for (int i = 0; i < n; i += 2) pairs += ea::pl_log_pair<HostOps>(s[i], i + 1 < n ? s[i + 1] : 1.0);
  st.renorms += renorms;
  ++st.runs;
  if (!std::isfinite(got)) { printf("FAIL %s, n = %d: not finite (%g)\n", kNames[c], n, got); return false; }
  if (ref == 0) {  // every factor exactly 1
    if (got != 0) { printf("FAIL %s, n = %d: factors all 1 give %g\n", kNames[c], n, got); return false; }
    return true;
  }
  const long double er = fabsl(got - ref) / ref, ep = fabsl(pairs - ref) / ref;
  if (er > st.worst_run) { st.worst_run = er; st.worst_n = n; }
  if (ep > st.worst_pairs) st.worst_pairs = ep;
  return true;
}

}  // namespace

int main() {
  const long double bar = 8 * ldexpl(1.0L, -53);
  const int ns[4] = {1, 2, 127, 128};
  bool ok = true;
  long double worst = 0;
  for (int c = 0; c < kCases && ok; ++c) {
    Stat st;
    long per_n_renorms[4] = {0, 0, 0, 0};
    for (int k = 0; k < 4 && ok; ++k) {
      std::vector<double> s((size_t)ns[k]);
      const long before = st.renorms;
      for (int rep = 0; rep < 2000 && ok; ++rep) {
        fill((Case)c, s);
        ok = measure((Case)c, s, st);
      }
      per_n_renorms[k] = st.renorms - before;
    }
    printf("%-24s %ld runs; worst relative error: running product %.3Le (n = %d), pairwise sum %.3Le; renormalisations %ld (n = 1: %ld, 2: %ld, 127: %ld, 128: %ld)\n",
           kNames[c], st.runs, st.worst_run, st.worst_n, st.worst_pairs, st.renorms, per_n_renorms[0], per_n_renorms[1],
           per_n_renorms[2], per_n_renorms[3]);
    if (st.worst_run > worst) worst = st.worst_run;
    if (ok && !(st.worst_run <= bar)) { printf("FAIL %s: above 8 * 2^-53 = %.3Le\n", kNames[c], bar); ok = false; }
    if (ok && c <= kTiny && st.renorms != 0) { printf("FAIL %s: renormalised with factors near 1\n", kNames[c]); ok = false; }
    if (ok && c >= kHuge && st.renorms == 0) { printf("FAIL %s: never renormalised\n", kNames[c]); ok = false; }
    // a single factor past the bound renormalises at every n
    if (ok && c >= kOne1e200)
      for (int k = 0; k < 4; ++k)
        if (per_n_renorms[k] < 2000) { printf("FAIL %s: n = %d, a run did not renormalise\n", kNames[c], ns[k]); ok = false; }
  }
  printf("worst over all cases: %.3Le (bar %.3Le)\n", worst, bar);
  printf(ok ? "ok\n" : "failed\n");
  return ok ? 0 : 1;
}
