// pair_log_host_shim.cpp — edge_alignment_amd/csrc/ea_pair_log.h on the CPU (tests/test_pair_log_host.py builds this under
// AddressSanitizer and UBSan and runs it): the header's text with host stand-ins for the device's operations, measured in
// long double.
//
// For arguments s = 1 + x as the Cauchy loss forms them, the sum of a pair of logarithms is taken three ways -- two
// separate logs (pl_log, what a lane with one point does), the paired log (pl_log_pair) and the paired log without its error
// term -- and each is compared with logl(s0) + logl(s1) of the two ROUNDED sums.  The bar: over the whole sweep the pair's
// worst relative error is at most twice the separate form's worst, measured in the same sweep; and the uncorrected form
// misses that same bar around x = 1e-8 (which is why the error term is there).
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
  static double rcp(double x) { return (double)(1.0f / (float)x); }
  static double sconst(double c) { return c; }
};

struct Worst { long double sep = 0, pair = 0, raw = 0; double at_pair[2] = {0, 0}; long n = 0; };

bool measure(double s0, double s1, Worst &w) {
  const long double ref = logl((long double)s0) + logl((long double)s1);
  const double sep = ea::pl_log<HostOps>(s0) + ea::pl_log<HostOps>(s1);
  const double pair = ea::pl_log_pair<HostOps>(s0, s1);
  const double raw = ea::pl_log_pair<HostOps, false>(s0, s1);
  ++w.n;
  if (ref == 0) {  // both arguments exactly 1: every form gives exactly 0
    if (sep != 0 || pair != 0 || raw != 0) { printf("FAIL log 1 + log 1: %g %g %g\n", sep, pair, raw); return false; }
    return true;
  }
  if (!std::isfinite(pair)) { printf("FAIL not finite: pair(%a, %a) = %g\n", s0, s1, pair); return false; }
  const long double es = fabsl(sep - ref) / ref, ep = fabsl(pair - ref) / ref, er = fabsl(raw - ref) / ref;
  if (es > w.sep) w.sep = es;
  if (ep > w.pair) { w.pair = ep; w.at_pair[0] = s0; w.at_pair[1] = s1; }
  if (er > w.raw) w.raw = er;
  return true;
}

// xorshift64*: the sweep is the same everywhere
uint64_t g_state = 0x9E3779B97F4A7C15ull;
double uniform01() {
  g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
  return (double)((g_state * 0x2545F4914F6CDD1Dull) >> 11) * (1.0 / 9007199254740992.0);
}
double log_uniform(double lo10, double hi10) { return std::pow(10.0, lo10 + (hi10 - lo10) * uniform01()); }

}  // namespace

int main() {
  bool ok = true;
  Worst all;
  // x log-uniform over the whole range, both members independent; then both members of one magnitude (the lanes of a
  // converged solve: two small residuals)
  for (int i = 0; i < 200000 && ok; ++i) ok = measure(1.0 + log_uniform(-300, 300), 1.0 + log_uniform(-300, 300), all);
  for (int i = 0; i < 200000 && ok; ++i) {
    const double d = -300 + 600 * uniform01();
    ok = measure(1.0 + log_uniform(d - 0.5, d + 0.5), 1.0 + log_uniform(d - 0.5, d + 0.5), all);
  }
  // x = 0 in one member or both, one member exactly 1
  for (int i = 0; i < 20000 && ok; ++i) {
    const double s = 1.0 + log_uniform(-300, 300);
    ok = measure(1.0 + 0.0, s, all) && measure(s, 1.0, all);
  }
  ok = ok && measure(1.0, 1.0, all);
  // both members, and their product, at the boundaries of the mantissa interval [sqrt(1/2), sqrt(2)) and of a binade
  {
    std::vector<double> edge;
    for (double c : {std::sqrt(2.0), 2.0 * std::sqrt(0.5), std::pow(2.0, 0.25), std::pow(2.0, 0.75), 2.0, 4.0, 2.0 * std::sqrt(2.0), 1.0}) {
      double lo = c, hi = c;
      for (int k = 0; k < 4; ++k) {
        edge.push_back(lo); edge.push_back(hi);
        lo = std::nextafter(lo, 0.0); hi = std::nextafter(hi, 1e300);
      }
    }
    for (double a : edge)
      for (double b : edge)
        if (a >= 1.0 && b >= 1.0 && ok) ok = measure(a, b, all);
    for (int i = 0; i < 100000 && ok; ++i) {  // a random member, its partner chosen so that the product lands on an edge
      const double a = 1.0 + log_uniform(-3, 2), c = edge[(size_t)(uniform01() * edge.size()) % edge.size()];
      double b = c * std::ldexp(1.0, (int)(20 * uniform01())) / a;
      while (b < 1.0) b *= 2.0;
      ok = measure(a, b, all);
    }
  }
  printf("sweep: %ld pairs; worst relative error: separate %.3Le, pair %.3Le (at %a, %a), pair without the error term %.3Le\n",
         all.n, all.sep, all.pair, all.at_pair[0], all.at_pair[1], all.raw);
  if (ok && !(all.pair <= 2 * all.sep)) { printf("FAIL pair above twice the separate form\n"); ok = false; }
  // the form without the error term, around x = 1e-8, against the same bar
  Worst small;
  for (int i = 0; i < 100000 && ok; ++i) ok = measure(1.0 + log_uniform(-8.3, -7.7), 1.0 + log_uniform(-8.3, -7.7), small);
  printf("x ~ 1e-8: %ld pairs; separate %.3Le, pair %.3Le, pair without the error term %.3Le\n", small.n, small.sep, small.pair, small.raw);
  if (ok && !(small.pair <= 2 * small.sep)) { printf("FAIL pair above twice the separate form at x ~ 1e-8\n"); ok = false; }
  if (ok && small.raw <= 2 * small.sep) { printf("FAIL the uncorrected form passes at x ~ 1e-8: the check has no teeth\n"); ok = false; }
  printf(ok ? "ok\n" : "failed\n");
  return ok ? 0 : 1;
}
