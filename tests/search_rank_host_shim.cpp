// The ranking of a search in front of the multi-start solve (edge_alignment_amd/csrc/ea_search_rank.h) swept on the host:
// count {1, 3} x K {1, 2, 9, 257} x M {1, K / 2, K} over random costs with planted exact ties, NaN and +-Inf, candidates with
// failed functors, every candidate ineligible, and exactly M - 1 eligible.  The result must equal a plain restatement of the
// rule -- a stable sort of the candidate indices by (ineligible, cost) -- and every column of `picked` must be a prefix of a
// permutation: in range, no repeats.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "ea_search_rank.h"

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

// the rule, restated: per problem a stable sort by (ineligible, cost of the eligible); index order breaks every tie
static std::vector<int> expected(int K, int M, int count, const std::vector<double> &cost, const std::vector<int64_t> &bad) {
  std::vector<int> out((size_t)M * count);
  for (int i = 0; i < count; ++i) {
    std::vector<int> idx((size_t)K);
    for (int k = 0; k < K; ++k) idx[(size_t)k] = k;
    auto inel = [&](int k) { const double c = cost[(size_t)k * count + i]; return !(std::isfinite(c) && bad[(size_t)k * count + i] == 0); };
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) {
      const bool ia = inel(a), ib = inel(b);
      if (ia != ib) return ib;
      if (ia) return false;
      return cost[(size_t)a * count + i] < cost[(size_t)b * count + i];
    });
    for (int m = 0; m < M; ++m) out[(size_t)m * count + i] = idx[(size_t)m];
  }
  return out;
}

// mode 0: random with ties, non-finite costs and failed functors; 1: every candidate ineligible; 2: exactly M - 1 eligible
static void sweep(int count, int K, int M, int mode, int round) {
  const size_t n = (size_t)K * count;
  std::vector<double> cost(n);
  std::vector<int64_t> bad(n, 0);
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  for (size_t s = 0; s < n; ++s) cost[s] = 1.0 + 100.0 * rnd01();
  for (int i = 0; i < count; ++i) {
    auto at = [&](int k) { return (size_t)k * count + i; };
    if (mode == 0) {
      for (int k = 0; k < K; ++k) {
        const unsigned r = (unsigned)(rnd() % 16);
        if (r == 0) cost[at(k)] = nan;
        else if (r == 1) cost[at(k)] = inf;
        else if (r == 2) cost[at(k)] = -inf;
        else if (r == 3) bad[at(k)] = 1 + (int64_t)(rnd() % 5);
        else if (r < 8 && k > 0) cost[at(k)] = cost[at((int)(rnd() % (unsigned)k))];  // an exact tie with an earlier candidate
        else if (r == 8) cost[at(k)] = 0.0;
        else if (r == 9) cost[at(k)] = -0.0;
      }
    } else if (mode == 1) {
      for (int k = 0; k < K; ++k) {
        if ((k + round) % 3 == 0) cost[at(k)] = nan;
        else if ((k + round) % 3 == 1) bad[at(k)] = 2;
        else cost[at(k)] = (k & 1) ? inf : -inf;
      }
    } else {
      // M - 1 eligible candidates at scattered indices, the rest fail
      std::vector<int> idx((size_t)K);
      for (int k = 0; k < K; ++k) idx[(size_t)k] = k;
      for (int k = K - 1; k > 0; --k) std::swap(idx[(size_t)k], idx[(size_t)(rnd() % (unsigned)(k + 1))]);
      for (int j = M - 1; j < K; ++j) {
        if (j & 1) bad[at(idx[(size_t)j])] = 1; else cost[at(idx[(size_t)j])] = nan;
      }
    }
  }
  std::vector<int> picked((size_t)M * count + 2, -7);  // (guards either side of the output)
  search_rank(K, M, count, cost.data(), bad.data(), picked.data() + 1);
  REQUIRE(picked.front() == -7 && picked.back() == -7);
  const std::vector<int> want = expected(K, M, count, cost, bad);
  for (int i = 0; i < count; ++i) {
    std::vector<char> seen((size_t)K, 0);
    int eligible = 0;
    for (int k = 0; k < K; ++k) eligible += search_eligible(cost[(size_t)k * count + i], bad[(size_t)k * count + i]) ? 1 : 0;
    if (mode == 1) REQUIRE(eligible == 0);
    if (mode == 2) REQUIRE(eligible == M - 1);
    for (int m = 0; m < M; ++m) {
      const int k = picked[1 + (size_t)m * count + i];
      REQUIRE(k >= 0 && k < K);
      REQUIRE(!seen[(size_t)k]);
      seen[(size_t)k] = 1;
      REQUIRE(k == want[(size_t)m * count + i]);
      REQUIRE(search_eligible(cost[(size_t)k * count + i], bad[(size_t)k * count + i]) == (m < eligible));
    }
  }
}

int main() {
  int cases = 0;
  const int counts[] = {1, 3}, Ks[] = {1, 2, 9, 257};
  for (int count : counts)
    for (int K : Ks) {
      const int Ms[] = {1, std::max(1, K / 2), K};
      for (int M : Ms)
        for (int mode = 0; mode < 3; ++mode)
          for (int round = 0; round < 6; ++round) { sweep(count, K, M, mode, round); ++cases; }
    }
  // the argument rule of ea_batch_search_starts
  REQUIRE(search_rank_args_ok(1, 1, 1) && search_rank_args_ok(16384, 16384, 1) && search_rank_args_ok(9, 4, 4096));
  REQUIRE(!search_rank_args_ok(4, 0, 1) && !search_rank_args_ok(4, -1, 1) && !search_rank_args_ok(4, 5, 1));
  REQUIRE(!search_rank_args_ok(20000, 16385, 1) && !search_rank_args_ok(9, 5, 4096) && !search_rank_args_ok(1 << 20, 1 << 20, 1 << 12));
  std::printf("ok %d cases %lld checks\n", cases, checks);
  return 0;
}
