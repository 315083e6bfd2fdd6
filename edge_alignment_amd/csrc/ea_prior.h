// ea_prior.h -- ceres::NormalPrior on the pose blocks (Ceres <= 2.1), folded into the 32 accumulator slots.  Host/device
// (EA_HD) fp64 code: the LM kernels of ea_kernels.hip run it on the state machine's lane, the host drivers of ea_capi.hip on
// the folded sums they hand back or all-reduce, tests/prior_host_shim.cpp compiles it with g++ for the CPU suite.
//
// A NormalPrior(A, b) on one parameter block x (q: ambient 4, t: 3) has residual r = A (x - b), cost 1/2 |A (x - b)|^2, no
// loss function, and tangent Jacobian A P(q) on q (P = QuaternionParameterization::ComputeJacobian, 4x3), A on t.  What it
// adds to the accumulator, with H = A^T A (formed once on the host in fp64 and stored with b -- a documented deviation from
// keeping A, at rounding level) and d = x - b:
//   q:  JtJ[dd] += P^T H P,   Jtr[d] += P^T H d,   cost += 1/2 d^T H d
//   t:  JtJ[tt] += H,         Jtr[t] += H d,       cost += 1/2 d^T H d
// Every index is a constant: the small matrices stay in registers (no scratch on the device).
#pragma once
#include <stdint.h>

#include "ea_types.h"

namespace ea {

#if defined(__clang__)
#define EA_PRIOR_UNROLL _Pragma("unroll")
#else
#define EA_PRIOR_UNROLL
#endif

// One pose's priors; a block whose flag is 0 contributes nothing (its H and b are not read).  Indexed like GroupDesc /
// PoseState (one per problem of a batch), in a table of its own: ProblemDesc stays as the evaluation kernels fetch it.
struct PriorDesc {
  double Hq[16];  // A^T A of the quaternion block, 4x4 row-major
  double bq[4];
  double Ht[9];   // A^T A of the translation block, 3x3 row-major
  double bt[3];
  int32_t has_q, has_t;
  // The side table's other passenger: the tangent coordinates the solve and the covariance hold constant (bit i = coordinate
  // i of [delta | t]; ea_problem_set_constant_parameters).  prior_add does not read it: priors enter first, the mask is
  // applied to the sums afterwards (lm_mask_system in ea_lm.h, cov_from_acc in ea_cov.h).
  int32_t held, pad_;
};

static_assert(sizeof(PriorDesc) % 8 == 0, "PriorDesc sits in an array of doubles-aligned records");

// packed upper-triangle index of (a, c), a <= c, of the 6x6 JtJ slots (ea_types.h)
EA_HD constexpr int prior_sym6(int a, int c) { return a * 6 - a * (a - 1) / 2 + (c - a); }

// the priors' terms at x = (q, t) added to acc (JtJ, Jtr, cost); the other slots are untouched
EA_HD inline void prior_add(const PriorDesc &pr, const double x[7], double acc[kAccSlots]) {
  if (pr.has_q) {
    double d[4], Hd[4];
    EA_PRIOR_UNROLL
    for (int i = 0; i < 4; ++i) d[i] = x[i] - pr.bq[i];
    double c = 0.0;
    EA_PRIOR_UNROLL
    for (int i = 0; i < 4; ++i) {
      double s = 0.0;
      EA_PRIOR_UNROLL
      for (int k = 0; k < 4; ++k) s += pr.Hq[4 * i + k] * d[k];
      Hd[i] = s;
      c += d[i] * s;
    }
    // P(q), 4x3 row-major (QuaternionParameterization::ComputeJacobian at q as given)
    const double P[12] = {-x[1], -x[2], -x[3], x[0], x[3], -x[2], -x[3], x[0], x[1], x[2], -x[1], x[0]};
    double HP[12];  // H P
    EA_PRIOR_UNROLL
    for (int i = 0; i < 4; ++i)
      EA_PRIOR_UNROLL
      for (int j = 0; j < 3; ++j) {
        double s = 0.0;
        EA_PRIOR_UNROLL
        for (int k = 0; k < 4; ++k) s += pr.Hq[4 * i + k] * P[3 * k + j];
        HP[3 * i + j] = s;
      }
    EA_PRIOR_UNROLL
    for (int a = 0; a < 3; ++a) {
      double g = 0.0;
      EA_PRIOR_UNROLL
      for (int i = 0; i < 4; ++i) g += P[3 * i + a] * Hd[i];
      acc[kAccJtr + a] += g;
      EA_PRIOR_UNROLL
      for (int b = a; b < 3; ++b) {
        double s = 0.0;
        EA_PRIOR_UNROLL
        for (int i = 0; i < 4; ++i) s += P[3 * i + a] * HP[3 * i + b];
        acc[kAccJtJ + prior_sym6(a, b)] += s;
      }
    }
    acc[kAccCost] += 0.5 * c;
  }
  if (pr.has_t) {
    double d[3];
    EA_PRIOR_UNROLL
    for (int i = 0; i < 3; ++i) d[i] = x[4 + i] - pr.bt[i];
    double c = 0.0;
    EA_PRIOR_UNROLL
    for (int a = 0; a < 3; ++a) {
      double s = 0.0;
      EA_PRIOR_UNROLL
      for (int k = 0; k < 3; ++k) s += pr.Ht[3 * a + k] * d[k];
      acc[kAccJtr + 3 + a] += s;
      c += d[a] * s;
      EA_PRIOR_UNROLL
      for (int b = a; b < 3; ++b) acc[kAccJtJ + prior_sym6(3 + a, 3 + b)] += pr.Ht[3 * a + b];
    }
    acc[kAccCost] += 0.5 * c;
  }
}

}  // namespace ea
