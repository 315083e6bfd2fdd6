// ea_search_rank.h — which of K candidate poses per problem a ranked search hands to the multi-start solve
// (ea_batch_search_starts), as a pure host function: the library calls it on the results of the cost-only evaluation, and
// tests sweep it without a device (tests/search_rank_host_shim.cpp).
//
// Candidate k of problem i has cost[k * count + i] and n_invalid[k * count + i] (the layout of ea_batch_cost_poses).  It is
// ELIGIBLE if its cost is finite and none of its functors failed: a start whose functor fails ends EA_WHY_INITIAL_EVAL_FAILED
// under Ceres' rule anyway, and a sum over fewer points is a smaller sum -- it would rank unfairly.  Ranks of a problem: the
// eligible candidates by ascending cost, ties to the lower candidate index; the ineligible ones behind them by ascending
// index.  picked[m * count + i] = the candidate of rank m for problem i, m < M.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "ea_starts_map.h"

namespace ea {

// 1 <= M <= K and M x count starts fit one multi-start solve
inline bool search_rank_args_ok(int K, int M, int count) {
  return count >= 1 && M >= 1 && M <= K && (int64_t)M * count <= kMaxStartSlots;
}

inline bool search_eligible(double cost, int64_t n_invalid) { return std::isfinite(cost) && n_invalid == 0; }

inline void search_rank(int K, int M, int count, const double *cost, const int64_t *n_invalid, int *picked) {
  std::vector<int> order((size_t)K);
  for (int i = 0; i < count; ++i) {
    auto at = [&](int k) { return (size_t)k * count + i; };
    // eligible candidates to the front, both parts in index order; then the front by (cost, index)
    int ne = 0;
    for (int k = 0; k < K; ++k) if (search_eligible(cost[at(k)], n_invalid[at(k)])) order[(size_t)ne++] = k;
    int tail = ne;
    for (int k = 0; k < K; ++k) if (!search_eligible(cost[at(k)], n_invalid[at(k)])) order[(size_t)tail++] = k;
    std::partial_sort(order.begin(), order.begin() + std::min(M, ne), order.begin() + ne, [&](int a, int b) {
      const double ca = cost[at(a)], cb = cost[at(b)];
      return ca < cb || (ca == cb && a < b);
    });
    for (int m = 0; m < M; ++m) picked[(size_t)m * count + i] = order[(size_t)m];
  }
}

}  // namespace ea
