// ea_select.h — exact order statistics of |r| by radix select, the part that is pure logic: shared by the select kernels
// (ea_kernels.hip), the host driver (ea_segments.hip) and a host sweep without a device (tests/select_host_shim.cpp).
//
// A non-negative double orders as its bit pattern, so |r| is selected as a 64-bit key, most significant digit first: six
// passes, five of 11 bits and a last one of 9.  A pass counts, per (segment, quantile), the keys that still agree with the
// quantile's prefix by their digit (integer counts: the result does not depend on the order of arrival), and a scan turns the
// histogram and the rank into the digit to append and the rank among the keys of that bin.  After the last pass the prefix IS
// the key at the rank -- an element of the multiset, not an interpolated value.  A block whose functor fails gets the all-ones
// key: it sorts behind every residual (behind +Inf and every NaN pattern of a sign-cleared double) and no rank reaches it.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "ea_types.h"

namespace ea {

constexpr int kSelectMaxQ = 16;          // quantiles per call
constexpr int kSelectPasses = 6;
constexpr int kSelectDigitBits = 11;
constexpr int kSelectBins = 1 << kSelectDigitBits;
constexpr int kSelectThreads = 256;      // workgroup size of every select kernel
constexpr int kSelectKeysPerLane = 8;    // histogram pass: keys per lane
constexpr int kSelectChunk = kSelectThreads * kSelectKeysPerLane;
constexpr uint64_t kSelectFailedKey = ~(uint64_t)0;

// one segment of the key array = the residual family of one problem: keys [begin, begin + n); term = its descriptor
struct SelectSeg {
  int64_t begin;
  int32_t n;
  int32_t term;
};

// ea_batch_pose_stats (ea_pose_stats_kernel) walks the same segments, `begin` being the segment's first partial row: one row
// per workgroup of kPoseStatsThreads points, folded in index order into one PoseStatsRow (= ea_pose_stats) per segment
constexpr int kPoseStatsThreads = 256;
struct PoseStatsPartial {
  int32_t n_invalid, n_visible, n_inlier, n_flow;
  double sum_flow, pad_;
};
struct PoseStatsRow {
  int64_t n, n_invalid, n_visible, n_inlier, n_flow;
  double sum_flow;
};
EA_HD inline int64_t pose_stats_rows(int64_t n) { return (n + kPoseStatsThreads - 1) / kPoseStatsThreads; }

EA_HD inline uint64_t select_bits(double v) { uint64_t u; memcpy(&u, &v, sizeof u); return u; }
EA_HD inline double select_value(uint64_t key) { double v; memcpy(&v, &key, sizeof v); return v; }
// key of the residual of a block whose functor succeeded: the bits of |r|
EA_HD inline uint64_t select_key_abs(double r) { return select_bits(r) & ~((uint64_t)1 << 63); }
// key of a caller-supplied value (ea_selftest_select): NaN = a failed block, everything else by absolute value
EA_HD inline uint64_t select_key(double v) { return v != v ? kSelectFailedKey : select_key_abs(v); }

// pass p looks at bits [shift, shift + 11) -- the last one at the 9 bits that are left
EA_HD inline int select_shift(int pass) { return pass < kSelectPasses - 1 ? 64 - kSelectDigitBits * (pass + 1) : 0; }
EA_HD inline unsigned select_digit(uint64_t key, int pass) {
  return (unsigned)(key >> select_shift(pass)) & (unsigned)(pass < kSelectPasses - 1 ? kSelectBins - 1 : (1 << 9) - 1);
}
// does `key` agree with `prefix` in every digit of the passes before `pass`
EA_HD inline bool select_matches(uint64_t key, uint64_t prefix, int pass) {
  if (pass == 0) return true;
  const int s = select_shift(pass - 1);
  return (key >> s) == (prefix >> s);
}
EA_HD inline uint64_t select_extend(uint64_t prefix, int pass, unsigned bin) { return prefix | ((uint64_t)bin << select_shift(pass)); }
// Quantiles whose prefixes agree so far look at the same keys: only the first of them (the leader) has a histogram built.
EA_HD inline int select_leader(const uint64_t *prefix, int q, int pass) {
  for (int j = 0; j < q; ++j)
    if (select_matches(prefix[j], prefix[q], pass)) return j;
  return q;
}

// rank of a probability among m valid blocks: floor(prob * (m - 1)), one IEEE multiplication (numpy's method="lower")
EA_HD inline int64_t select_rank(double prob, int64_t m) {
  if (m <= 0) return 0;
  const double x = prob * (double)(m - 1);
  int64_t k = (int64_t)floor(x);
  if (k < 0) k = 0;
  if (k > m - 1) k = m - 1;
  return k;
}

// histogram + rank -> the bin that holds the rank-th count and the rank inside that bin.  The counts may be of any unsigned
// type (a bin, or the sum of a group of bins).  A rank past the total ends in the last bin with rank 0 (empty segments).
template <typename C>
EA_HD inline int select_scan(const C *hist, int nbins, int64_t rank, int64_t *remaining) {
  int64_t below = 0;
  for (int b = 0; b < nbins; ++b) {
    const int64_t c = (int64_t)hist[b];
    if (rank < below + c) { *remaining = rank - below; return b; }
    below += c;
  }
  *remaining = 0;
  return nbins - 1;
}

// The number of valid blocks of a segment, read off the histogram of pass 0: a valid key has the sign bit clear, so its first
// digit is below 1024, and the failed key's is 2047.  group_sums: the 16 sums of 128 consecutive bins each.
template <typename C>
EA_HD inline int64_t select_valid_count(const C *group_sums) {
  int64_t m = 0;
  for (int g = 0; g < 8; ++g) m += (int64_t)group_sums[g];
  return m;
}

// the loss scale of ea_problem_set_loss_auto_scale: a = max(a_min, factor * Q), one IEEE multiplication; a NaN quantile
// gives a_min
EA_HD inline double select_loss_scale(double factor, double Q, double a_min) {
  const double a = factor * Q;
  return a > a_min ? a : a_min;
}

inline bool select_prob_ok(double prob) { return prob >= 0.0 && prob <= 1.0; }  // (NaN fails both)

}  // namespace ea
