// ea_cov.h -- pose covariance from the 6x6 normal equations (ceres::Covariance <= 2.1, one pose, tangent ordering
// [delta(3) | t(3)]).  Host/device (EA_HD) fp64 code: the covariance kernel of ea_capi.hip runs it on one lane per
// problem, tests/cov_host_shim.cpp compiles the same header with g++ for the CPU suite.
//
//   JtJ = sum rho' J J^T (or sum J J^T with the loss off) -> eigenvalues lambda_1 >= ... >= lambda_6 (cyclic Jacobi)
//   -> rank decision (Ceres' DENSE_SVD rule restated on lambda_i = sigma_i^2) -> C = sum_{kept} v v^T / lambda
//   -> ambient blocks through the quaternion parameterisation's 4x3 Jacobian L at q as given (not normalised).
//
// SPARSE_QR: Ceres decides full rank by SuiteSparseQR's column-norm tolerance; here it is the DENSE_SVD test with
// null_space_rank = 0 (lambda_6 / lambda_1 >= min_reciprocal_condition_number) -- a documented deviation, identical on
// every well-determined pose, possibly different on a nearly rank-deficient one.
#pragma once
#include <math.h>

#include "../../include/ea_hip.h"
#include "ea_types.h"

namespace ea {

// Every loop over matrix indices is unrolled: with constant indices the 6x6 arrays live in registers (a dynamically indexed
// array goes to scratch memory, and one lane's chain of scratch round trips is what the decomposition would then cost).
#if defined(__clang__)
#define EA_COV_UNROLL _Pragma("unroll")
#else
#define EA_COV_UNROLL
#endif

constexpr int kCovSweeps = 32;  // cyclic Jacobi sweeps at most (a 6x6 SPD system converges in 6-8)

struct CovOptions {
  int algorithm;                  // EA_COV_SPARSE_QR | EA_COV_DENSE_SVD
  double min_rcn;                 // min_reciprocal_condition_number
  int null_space_rank;            // -1 = automatic truncation, 0..6 = exact number of dropped directions
};

// upper triangle of the accumulator slots (kAccJtJ.., row-major a <= b) -> full symmetric 6x6
EA_HD inline void cov_unpack_jtj(const double *acc, double A[36]) {
  int k = 0;
  EA_COV_UNROLL
  for (int a = 0; a < 6; ++a)
    EA_COV_UNROLL
    for (int c = a; c < 6; ++c) {
      A[6 * a + c] = acc[kAccJtJ + k];
      A[6 * c + a] = acc[kAccJtJ + k];
      ++k;
    }
}

// Symmetric eigen-decomposition by cyclic Jacobi rotations: lam descending, V (row-major) holds the eigenvector of lam[j]
// in column j.  A rotation is skipped when |a_pq| <= 1e-17 sqrt(|a_pp a_qq|) (the relative criterion that keeps small
// eigenvalues of a positive definite matrix accurate); the loop ends after a sweep without rotation or kCovSweeps sweeps.
// held (bit i = tangent coordinate i constant): the decomposition of the REDUCED matrix over the free coordinates.  The held
// rows and columns are exact zeros, so no rotation ever touches them -- the rotations are those of the cyclic Jacobi method on
// the m x m sub-matrix, in its order -- and their eigenpairs (0, e_i) are sorted behind the m free ones whatever the sign of
// a free eigenvalue: lam holds the sub-matrix's m eigenvalues, descending, then zeros, and no placeholder takes part in the
// rank rule.  held = 0 is the code without the parameter.
EA_HD inline void cov_eigh(const double Ain[36], double lam[6], double V[36], int held = 0) {
  double A[36];
  EA_COV_UNROLL
  for (int i = 0; i < 36; ++i) {
    A[i] = (((held >> (i / 6)) | (held >> (i % 6))) & 1) ? 0.0 : Ain[i];
    V[i] = (i % 7 == 0) ? 1.0 : 0.0;
  }
  for (int sweep = 0; sweep < kCovSweeps; ++sweep) {
    int rotated = 0;
    EA_COV_UNROLL
    for (int p = 0; p < 5; ++p)
      EA_COV_UNROLL
      for (int q = p + 1; q < 6; ++q) {
        const double apq = A[6 * p + q], app = A[6 * p + p], aqq = A[6 * q + q];
        if (apq == 0.0 || fabs(apq) <= 1e-17 * sqrt(fabs(app * aqq))) {
          A[6 * p + q] = A[6 * q + p] = 0.0;
          continue;
        }
        rotated = 1;
        const double theta = (aqq - app) / (2.0 * apq);
        double t;
        if (fabs(theta) > 1e150) t = 0.5 / theta;
        else t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        EA_COV_UNROLL
        for (int k = 0; k < 6; ++k) {  // A <- A P (columns p, q)
          const double akp = A[6 * k + p], akq = A[6 * k + q];
          A[6 * k + p] = c * akp - s * akq;
          A[6 * k + q] = s * akp + c * akq;
        }
        EA_COV_UNROLL
        for (int k = 0; k < 6; ++k) {  // A <- P^T A (rows p, q)
          const double apk = A[6 * p + k], aqk = A[6 * q + k];
          A[6 * p + k] = c * apk - s * aqk;
          A[6 * q + k] = s * apk + c * aqk;
        }
        A[6 * p + q] = A[6 * q + p] = 0.0;
        EA_COV_UNROLL
        for (int k = 0; k < 6; ++k) {  // V <- V P
          const double vkp = V[6 * k + p], vkq = V[6 * k + q];
          V[6 * k + p] = c * vkp - s * vkq;
          V[6 * k + q] = s * vkp + c * vkq;
        }
      }
    if (!rotated) break;
  }
  double d[6];
  bool h[6];  // column j is a held coordinate's (0, e_j)
  EA_COV_UNROLL
  for (int i = 0; i < 6; ++i) { d[i] = A[7 * i]; h[i] = ((held >> i) & 1) != 0; }
  EA_COV_UNROLL
  for (int i = 0; i < 5; ++i)  // bubble network, descending, columns of V along (fixed indices: selects, no scratch)
    EA_COV_UNROLL
    for (int j = 0; j < 5 - i; ++j)
      if (h[j] != h[j + 1] ? h[j] : d[j] < d[j + 1]) {
        const double tl = d[j]; d[j] = d[j + 1]; d[j + 1] = tl;
        const bool th = h[j]; h[j] = h[j + 1]; h[j + 1] = th;
        EA_COV_UNROLL
        for (int k = 0; k < 6; ++k) { const double tv = V[6 * k + j]; V[6 * k + j] = V[6 * k + j + 1]; V[6 * k + j + 1] = tv; }
      }
  EA_COV_UNROLL
  for (int i = 0; i < 6; ++i) lam[i] = d[i];
}

// Ceres' DenseSVD rule (covariance_impl.cc) on eigenvalues: max_rank = 6 - null_space_rank (6 when it is -1); for
// i < max_rank the ratio lambda_i / lambda_1 must reach min_rcn -- a failure ends the kept set when null_space_rank = -1
// and makes the covariance "not computed" otherwise.  SPARSE_QR: the same test with null_space_rank = 0.
// Returns the number of kept eigenpairs, or -1 for "not computed".  lambda_1 <= 0 (no information at all) is "not
// computed" unless nothing is to be kept.
// m: the size of the (reduced) system, lam[0 .. m) its eigenvalues -- max_rank = m - null_space_rank, SPARSE_QR asks for
// rank m.  m = 0 (every coordinate constant): nothing to compute, rank 0.
EA_HD inline int cov_rank(const double lam[6], const CovOptions &o, int m = 6) {
  const int nsr = o.algorithm == EA_COV_SPARSE_QR ? 0 : o.null_space_rank;
  const int max_rank = nsr < 0 ? m : m - nsr;
  if (max_rank <= 0) return 0;
  if (!(lam[0] > 0.0)) return nsr < 0 ? 0 : -1;
  int rank = 0;
  bool stop = false;
  EA_COV_UNROLL
  for (int i = 0; i < 6; ++i) {
    if (stop || i >= max_rank) continue;
    if (!(lam[i] / lam[0] >= o.min_rcn)) {
      if (nsr >= 0) return -1;
      stop = true;
      continue;
    }
    ++rank;
  }
  return rank;
}

// C = sum_{j < rank} V_j V_j^T / lam_j  (the pseudo-inverse over the kept eigenpairs; the inverse at full rank)
EA_HD inline void cov_pinv(const double lam[6], const double V[36], int rank, double C[36]) {
  EA_COV_UNROLL
  for (int a = 0; a < 6; ++a)
    EA_COV_UNROLL
    for (int c = a; c < 6; ++c) {
      double s = 0.0;
      EA_COV_UNROLL
      for (int j = 0; j < 6; ++j)
        if (j < rank) s += V[6 * a + j] * V[6 * c + j] / lam[j];
      C[6 * a + c] = s;
      C[6 * c + a] = s;
    }
}

// QuaternionParameterization::ComputeJacobian at q (w, x, y, z), 4x3 row-major
EA_HD inline void cov_quat_jacobian(const double q[4], double L[12]) {
  L[0] = -q[1]; L[1] = -q[2]; L[2] = -q[3];
  L[3] = q[0];  L[4] = q[3];  L[5] = -q[2];
  L[6] = -q[3]; L[7] = q[0];  L[8] = q[1];
  L[9] = q[2];  L[10] = -q[1]; L[11] = q[0];
}

// ambient blocks of GetCovarianceBlock: qq = L C_dd L^T (4x4), qt = L C_dt (4x3), tt = C_tt (3x3), all row-major
EA_HD inline void cov_lift(const double q[4], const double C[36], double qq[16], double qt[12], double tt[9]) {
  double L[12];
  cov_quat_jacobian(q, L);
  double LC[12];  // L C_dd
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 3; ++j) {
      double s = 0.0, u = 0.0;
      for (int k = 0; k < 3; ++k) { s += L[3 * i + k] * C[6 * k + j]; u += L[3 * i + k] * C[6 * k + 3 + j]; }
      LC[3 * i + j] = s;
      qt[3 * i + j] = u;
    }
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      double s = 0.0;
      for (int k = 0; k < 3; ++k) s += LC[3 * i + k] * L[3 * j + k];
      qq[4 * i + j] = s;
    }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) tt[3 * i + j] = C[6 * (3 + i) + 3 + j];
}

// One problem's covariance from its 32 accumulator slots (ea_eval's sums at pose q) into the public result struct.
// points = rows the evaluation covered (0: "no points", why 3).  The result is built in a local copy and stored once: on
// the device `out` is pinned host memory, where every read of a field already written would be a round trip over PCIe.
// held: the tangent coordinates that are constant (ea_problem_set_constant_parameters) -- decomposition and rank rule run on
// the reduced system, `tangent` has zero rows and columns there and the ambient blocks are lifted from it (a constant block
// gives zero blocks); with all six held ok = 1, rank = 0 and everything is zero.
EA_HD inline void cov_from_acc(const double *acc, const double q[4], int64_t points, const CovOptions &o, ea_covariance *out,
                               int held = 0) {
  ea_covariance r;
  r.ok = 0; r.why = 0; r.rank = 0;
  r.n_invalid = (int64_t)llround(acc[kAccInvalid]);
  r.cost = acc[kAccCost];
  for (int i = 0; i < 6; ++i) r.eigenvalues[i] = 0.0;
  for (int i = 0; i < 36; ++i) r.tangent[i] = 0.0;
  for (int i = 0; i < 16; ++i) r.qq[i] = 0.0;
  for (int i = 0; i < 12; ++i) r.qt[i] = 0.0;
  for (int i = 0; i < 9; ++i) r.tt[i] = 0.0;
  if (points <= 0) {
    r.why = 3;
  } else {
    double A[36], V[36];
    cov_unpack_jtj(acc, A);
    int m = 6;
    EA_COV_UNROLL
    for (int i = 0; i < 6; ++i) m -= (held >> i) & 1;
    cov_eigh(A, r.eigenvalues, V, held);
    const int rank = r.n_invalid > 0 ? -2 : cov_rank(r.eigenvalues, o, m);
    if (rank == -2) {
      r.why = 2;  // Ceres fails the Jacobian evaluation
    } else if (rank < 0) {
      r.why = 1;
    } else {
      r.rank = rank;
      cov_pinv(r.eigenvalues, V, rank, r.tangent);
      cov_lift(q, r.tangent, r.qq, r.qt, r.tt);
      r.ok = 1;
    }
  }
  *out = r;
}

}  // namespace ea
