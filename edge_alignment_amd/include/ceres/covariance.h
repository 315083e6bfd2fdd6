// ceres::Covariance (Ceres <= 2.1) for the problems the facade hosts: one (quaternion, translation) pose shared by every
// residual block.  Compute() builds the GPU problem(s) from the blocks the way ceres::Solve does (several residual
// families -> one problem with terms) and calls ea_problem_covariance at the parameter blocks' current values; the
// decomposition, the rank rule, the inverse and the ambient lift run on the device (include/ea_hip.h).
// Deviation: SPARSE_QR decides full rank by lambda_min / lambda_max >= min_reciprocal_condition_number on JtJ (the
// DENSE_SVD test with null_space_rank = 0), not by SuiteSparseQR's column-norm tolerance.  Included from ceres.h.
#ifndef EA_CERES_COVARIANCE_H
#define EA_CERES_COVARIANCE_H

#include <cstring>
#include <utility>
#include <vector>

#include "ceres.h"

namespace ceres {

// SUITE_SPARSE_QR / EIGEN_SPARSE_QR: the spellings of Ceres 1.x, the same algorithm here
enum CovarianceAlgorithmType { DENSE_SVD, SPARSE_QR, SUITE_SPARSE_QR = SPARSE_QR, EIGEN_SPARSE_QR = SPARSE_QR };

class Covariance {
 public:
  struct Options {
    CovarianceAlgorithmType algorithm_type = SPARSE_QR;
    double min_reciprocal_condition_number = 1e-14;
    int null_space_rank = 0;
    int num_threads = 1;               // accepted, ignored (the work is one 6x6 system on the device)
    bool apply_loss_function = true;
    // not part of Ceres: arithmetic type of the per-point evaluation and the GPU to use
    int ea_dtype = EA_F64;
    int ea_device = 0;
  };

  explicit Covariance(const Options &options) : options_(options) {}
  Covariance(const Covariance &) = delete;
  Covariance &operator=(const Covariance &) = delete;

  bool Compute(const std::vector<std::pair<const double *, const double *>> &covariance_blocks, Problem *problem) {
    requested_.clear();
    computed_ = false;
    double *q = nullptr, *t = nullptr;
    if (!problem || !ProblemAccess::PoseBlocks(problem, &q, &t)) return false;
    q_ = q; t_ = t;
    for (const auto &pr : covariance_blocks)
      if (Size(pr.first) == 0 || Size(pr.second) == 0) return false;  // not a parameter block of this problem
    std::vector<ea_problem *> ps;
    std::vector<std::vector<int>> order;
    std::string err;
    int rc = ProblemAccess::Build(problem, options_.ea_dtype, options_.ea_device, &ps, &order, &err);
    ea_covariance_options o;
    ea_default_covariance_options(&o);
    o.algorithm = options_.algorithm_type == DENSE_SVD ? EA_COV_DENSE_SVD : EA_COV_SPARSE_QR;
    o.min_reciprocal_condition_number = options_.min_reciprocal_condition_number;
    o.null_space_rank = options_.null_space_rank;
    o.apply_loss_function = options_.apply_loss_function ? 1 : 0;
    if (rc == EA_OK) rc = ea_problem_covariance(ps[0], q, t, &o, &result_);  // the problem with all its terms
    for (auto *p : ps)
      if (p) ea_problem_destroy(p);
    if (rc != EA_OK || !result_.ok) return false;
    requested_ = covariance_blocks;
    computed_ = true;
    return true;
  }

  // every pair of the given blocks
  bool Compute(const std::vector<const double *> &parameter_blocks, Problem *problem) {
    std::vector<std::pair<const double *, const double *>> pairs;
    for (size_t i = 0; i < parameter_blocks.size(); ++i)
      for (size_t j = i; j < parameter_blocks.size(); ++j) pairs.emplace_back(parameter_blocks[i], parameter_blocks[j]);
    return Compute(pairs, problem);
  }

  // ambient space: GlobalSize(a) x GlobalSize(b), row-major (the quaternion block through its parameterisation)
  bool GetCovarianceBlock(const double *a, const double *b, double *covariance_block) const {
    return Block(a, b, false, covariance_block);
  }
  // tangent space: LocalSize(a) x LocalSize(b)
  bool GetCovarianceBlockInTangentSpace(const double *a, const double *b, double *covariance_block) const {
    return Block(a, b, true, covariance_block);
  }
  // the blocks of the listed parameter blocks assembled into one row-major matrix (every pair must have been computed)
  bool GetCovarianceMatrix(const std::vector<const double *> &parameter_blocks, double *covariance_matrix) const {
    return Matrix(parameter_blocks, false, covariance_matrix);
  }
  bool GetCovarianceMatrixInTangentSpace(const std::vector<const double *> &parameter_blocks, double *covariance_matrix) const {
    return Matrix(parameter_blocks, true, covariance_matrix);
  }

  // not part of Ceres: the whole result of the last Compute (eigenvalues, rank, cost, why it was not computed)
  const ea_covariance &ea_result() const { return result_; }

 private:
  int Size(const double *p, bool tangent = false) const {
    if (p == q_) return tangent ? 3 : 4;
    if (p == t_) return 3;
    return 0;
  }
  bool Requested(const double *a, const double *b) const {
    for (const auto &pr : requested_)
      if ((pr.first == a && pr.second == b) || (pr.first == b && pr.second == a)) return true;
    return false;
  }
  bool Block(const double *a, const double *b, bool tangent, double *out) const {
    if (!computed_ || !out || !Requested(a, b)) return false;
    const int na = Size(a, tangent), nb = Size(b, tangent);
    if (tangent) {
      const int oa = a == q_ ? 0 : 3, ob = b == q_ ? 0 : 3;
      for (int i = 0; i < na; ++i)
        for (int j = 0; j < nb; ++j) out[nb * i + j] = result_.tangent[6 * (oa + i) + ob + j];
      return true;
    }
    for (int i = 0; i < na; ++i)
      for (int j = 0; j < nb; ++j) {
        double v;
        if (a == q_ && b == q_) v = result_.qq[4 * i + j];
        else if (a == q_) v = result_.qt[3 * i + j];
        else if (b == q_) v = result_.qt[3 * j + i];
        else v = result_.tt[3 * i + j];
        out[nb * i + j] = v;
      }
    return true;
  }
  bool Matrix(const std::vector<const double *> &blocks, bool tangent, double *out) const {
    if (!computed_ || !out) return false;
    int n = 0;
    for (const double *p : blocks) n += Size(p, tangent);
    int r0 = 0;
    for (const double *a : blocks) {
      int c0 = 0;
      for (const double *b : blocks) {
        double tmp[16];
        if (!Block(a, b, tangent, tmp)) return false;
        const int na = Size(a, tangent), nb = Size(b, tangent);
        for (int i = 0; i < na; ++i)
          for (int j = 0; j < nb; ++j) out[(size_t)n * (r0 + i) + c0 + j] = tmp[nb * i + j];
        c0 += nb;
      }
      r0 += Size(a, tangent);
    }
    return true;
  }

  Options options_;
  const double *q_ = nullptr, *t_ = nullptr;
  std::vector<std::pair<const double *, const double *>> requested_;
  bool computed_ = false;
  ea_covariance result_{};
};

}  // namespace ceres

#endif  // EA_CERES_COVARIANCE_H
