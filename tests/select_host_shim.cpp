// The radix select behind ea_*_residual_quantiles (edge_alignment_amd/csrc/ea_select.h) driven on the host: the header's key,
// digit, prefix match, leader, scan and rank rule run through the full six-pass selection, as the kernels run it -- per pass
// one histogram per leading quantile over the keys that still match its prefix, the scan in the kernels' three levels (16
// groups, 16 lanes, 8 bins) -- and the result is compared bit for bit with a plain sort of |v| written out here.
// Sizes {1, 2, 63, 64, 65, 257, 4099} x data {random, all equal, two values one ulp apart, +-0, denormals, 1e300 and +Inf,
// NaN dropped, all NaN} x probs {0, 0.25, 0.5, 1 - 2^-53, 1}; then the loss-scale rule with its a_min clamp.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "ea_select.h"

using namespace ea;

static long long checks = 0;
#define REQUIRE(c)                                                                   \
  do {                                                                               \
    ++checks;                                                                        \
    if (!(c)) { std::printf("FAILED %s line %d\n", #c, __LINE__); std::exit(1); }    \
  } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return rng_state;
}
static double rnd01() { return (double)(rnd() >> 11) * (1.0 / 9007199254740992.0); }
static uint64_t bits(double v) { uint64_t u; std::memcpy(&u, &v, 8); return u; }

// the selection as the kernels run it
static void select_passes(const std::vector<double> &v, const std::vector<double> &probs, std::vector<double> &out, int64_t &m) {
  const int nq = (int)probs.size();
  std::vector<uint64_t> keys(v.size());
  m = -1;  // (read off the first pass's histogram, as the scan kernel does)
  for (size_t i = 0; i < v.size(); ++i) keys[i] = select_key(v[i]);
  std::vector<uint64_t> prefix((size_t)nq, 0xdeadbeefdeadbeefull);  // (pass 0 must not look at it)
  std::vector<int64_t> rank((size_t)nq, -7);
  std::vector<unsigned> hist((size_t)nq * kSelectBins, 0u);
  for (int pass = 0; pass < kSelectPasses; ++pass) {
    std::vector<int> leader((size_t)nq);
    for (int q = 0; q < nq; ++q) leader[(size_t)q] = select_leader(prefix.data(), q, pass);
    for (int q = 0; q < nq; ++q) {
      if (leader[(size_t)q] != q) continue;
      for (uint64_t k : keys)
        if (select_matches(k, prefix[(size_t)q], pass)) {
          const unsigned d = select_digit(k, pass);
          REQUIRE(d < (unsigned)kSelectBins);
          hist[(size_t)q * kSelectBins + d]++;
        }
    }
    std::vector<uint64_t> next(prefix);
    for (int q = 0; q < nq; ++q) {
      const unsigned *h = hist.data() + (size_t)leader[(size_t)q] * kSelectBins;
      unsigned s1[256], s2[16];
      for (int l = 0; l < 256; ++l) { s1[l] = 0; for (int j = 0; j < 8; ++j) s1[l] += h[8 * l + j]; }
      for (int g = 0; g < 16; ++g) { s2[g] = 0; for (int j = 0; j < 16; ++j) s2[g] += s1[16 * g + j]; }
      if (pass == 0) {
        const int64_t mq = select_valid_count(s2);
        REQUIRE(q == 0 || mq == m);
        m = mq;
      }
      int64_t r = pass == 0 ? select_rank(probs[(size_t)q], m) : rank[(size_t)q];
      const int i2 = select_scan(s2, 16, r, &r);
      const int i1 = select_scan(s1 + 16 * i2, 16, r, &r);
      const int lane = 16 * i2 + i1;
      const int bin = 8 * lane + select_scan(h + 8 * lane, 8, r, &r);
      // the three-level walk is the flat scan
      int64_t r_flat = pass == 0 ? select_rank(probs[(size_t)q], m) : rank[(size_t)q];
      REQUIRE(select_scan(h, kSelectBins, r_flat, &r_flat) == bin && r_flat == r);
      next[(size_t)q] = select_extend(pass == 0 ? 0 : prefix[(size_t)q], pass, (unsigned)bin);
      rank[(size_t)q] = r;
    }
    prefix = next;
    for (int q = 0; q < nq; ++q)
      if (leader[(size_t)q] == q) std::fill(hist.begin() + (size_t)q * kSelectBins, hist.begin() + (size_t)(q + 1) * kSelectBins, 0u);
  }
  out.resize((size_t)nq);
  for (int q = 0; q < nq; ++q) out[(size_t)q] = m > 0 ? select_value(prefix[(size_t)q]) : std::numeric_limits<double>::quiet_NaN();
}

// the definition, restated: sort |v| of the values that are not NaN, take element floor(prob * (m - 1))
static void expected(const std::vector<double> &v, const std::vector<double> &probs, std::vector<double> &out, int64_t &m) {
  std::vector<double> a;
  for (double x : v) if (!(x != x)) a.push_back(std::fabs(x));
  std::sort(a.begin(), a.end());
  m = (int64_t)a.size();
  out.clear();
  for (double p : probs) {
    if (m == 0) { out.push_back(std::numeric_limits<double>::quiet_NaN()); continue; }
    const double x = p * (double)(m - 1);
    out.push_back(a[(size_t)std::floor(x)]);
  }
}

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const std::vector<double> probs = {0.0, 0.25, 0.5, 1.0 - std::ldexp(1.0, -53), 1.0};
  const int sizes[] = {1, 2, 63, 64, 65, 257, 4099};
  int cases = 0;
  // the pieces by themselves
  REQUIRE(select_key(-0.0) == 0 && select_key(0.0) == 0 && select_key(nan) == kSelectFailedKey && select_key(-nan) == kSelectFailedKey);
  REQUIRE(select_key(-1.5) == bits(1.5) && select_key(inf) < kSelectFailedKey && select_key(-inf) == bits(inf));
  REQUIRE(select_key(1.0) < select_key(std::nextafter(1.0, 2.0)) && select_key(5e-324) == 1);
  {
    uint64_t k = 0x123456789abcdef0ull, back = 0;
    for (int p = 0; p < kSelectPasses; ++p) back = select_extend(back, p, select_digit(k, p));
    REQUIRE(back == k);
    REQUIRE(select_shift(0) == 53 && select_shift(4) == 9 && select_shift(5) == 0);
  }
  REQUIRE(select_rank(0.5, 4) == 1 && select_rank(0.5, 5) == 2 && select_rank(1.0, 7) == 6 && select_rank(0.0, 7) == 0 && select_rank(0.3, 0) == 0);
  REQUIRE(select_rank(1.0 - std::ldexp(1.0, -53), 4099) == (int64_t)std::floor((1.0 - std::ldexp(1.0, -53)) * 4098.0));
  REQUIRE(select_prob_ok(0.0) && select_prob_ok(1.0) && !select_prob_ok(-0.1) && !select_prob_ok(1.1) && !select_prob_ok(nan));
  for (int n : sizes) {
    for (int kind = 0; kind < 8; ++kind) {
      std::vector<double> v((size_t)n);
      for (int i = 0; i < n; ++i) {
        double x = (rnd01() - 0.5) * std::exp(20.0 * (rnd01() - 0.5));
        switch (kind) {
          case 0: break;                                                           // random, both signs, many magnitudes
          case 1: x = -0.37; break;                                                // all equal
          case 2: x = (rnd() & 1) ? 1.0 : std::nextafter(1.0, 2.0); break;         // differ in the last mantissa bit: every pass
          case 3: x = (rnd() & 1) ? 0.0 : -0.0; break;                             // +-0
          case 4: x = (double)(rnd() % 1000) * 5e-324 * ((rnd() & 1) ? 1 : -1); break;  // denormals
          case 5: x = (i % 3 == 0) ? 1e300 : (i % 3 == 1 ? inf : -x); break;       // 1e300, +Inf
          case 6: if (rnd() % 3 == 0) x = nan; break;                              // NaN dropped
          case 7: x = nan; break;                                                  // all-NaN segment
        }
        v[(size_t)i] = x;
      }
      std::vector<double> got, want;
      int64_t m_got = -1, m_want = -2;
      select_passes(v, probs, got, m_got);
      expected(v, probs, want, m_want);
      REQUIRE(m_got == m_want);
      for (size_t q = 0; q < probs.size(); ++q) {
        if (m_want == 0) REQUIRE(got[q] != got[q]);
        else REQUIRE(bits(got[q]) == bits(want[q]));
      }
      ++cases;
    }
  }
  // loss scale: one multiplication, clamped from below; a NaN quantile gives a_min
  REQUIRE(select_loss_scale(2.385, 0.25, 1e-6) == 2.385 * 0.25);
  REQUIRE(select_loss_scale(2.385, 0.0, 1e-6) == 1e-6);
  REQUIRE(select_loss_scale(2.385, 1e-9, 1e-6) == 1e-6);
  REQUIRE(select_loss_scale(1.0, 1e-6, 1e-6) == 1e-6);
  REQUIRE(select_loss_scale(3.0, nan, 0.5) == 0.5);
  REQUIRE(select_loss_scale(0.1, 3.0, 1e-6) == 0.1 * 3.0);
  std::printf("ok %d cases %lld checks\n", cases, checks);
  return 0;
}
