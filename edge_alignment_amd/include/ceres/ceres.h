// ceres/ceres.h — the slice of the ceres:: API that kuwt/edge_alignment touches on its hot path,
// re-hosted on the MI355X C-ABI (include/ea_hip.h).  NOT Ceres Solver and not a general solver:
// a source-compatibility facade so that the reference's "Setup non-linear Least Squares" blocks
// (standalone/standalone_edge_align.cpp:256-293, src/SolveEA.cpp:124-216) compile and run
// unchanged against libea_hip.so.
//
// What it understands: residual blocks created by EAResidue::Create(...) /
// AutoDiffCostFunction<EAResidue,1,4,3> over ONE interpolator and ONE (q,t) pair, an optional
// CauchyLoss / HuberLoss / TrivialLoss (NULL = trivial), QuaternionParameterization on q, and the
// Solver::Options fields the reference sets.  Anything else is reported through
// Summary::termination_type = FAILURE with a message; nothing is evaluated on the CPU.
#pragma once

#include <cmath>
#include <cstdio>
#include <memory>
#include <sstream>
#include <string>
#include <algorithm>
#include <unordered_set>
#include <vector>

#include "../../../include/ea_hip.h"
#include "cubic_interpolation.h"
#include "jet.h"
#include "loss_function.h"
#include "rotation.h"

namespace ceres {

enum LinearSolverType { DENSE_NORMAL_CHOLESKY, DENSE_QR, SPARSE_NORMAL_CHOLESKY, DENSE_SCHUR, SPARSE_SCHUR, ITERATIVE_SCHUR, CGNR };
enum MinimizerType { LINE_SEARCH, TRUST_REGION };
enum TrustRegionStrategyType { LEVENBERG_MARQUARDT, DOGLEG };
enum DoglegType { TRADITIONAL_DOGLEG, SUBSPACE_DOGLEG };
enum TerminationType { CONVERGENCE, NO_CONVERGENCE, FAILURE, USER_SUCCESS, USER_FAILURE };

// ---- cost functions ------------------------------------------------------------------------
// The facade never differentiates anything: a cost function is only a carrier of the per-block
// constants (3-D point, intrinsics, interpolator) that the GPU kernels consume.
struct EABlockInfo {
  double fx, fy, cx, cy;
  double X, Y, Z;
  const double *grid_data;  // Grid2D view the functor samples at (r = u, c = v)
  int grid_rows, grid_cols;
  double z_guard, z_eps;    // functor flavour (standalone: 0.01, 0; ROS: 0, 0.001)
  int rot_transposed;
  // residual variants (utils.h:102-421); zero-initialised = plain EAResidue
  int variant = 0;          // bit 0: distortion (k1,k2,p1,p2,k3), bit 1: second camera (T12, T12inv)
  double dist[5] = {0, 0, 0, 0, 0};
  double T12[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  double T12inv[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
};

class NormalPrior;

class CostFunction {
 public:
  virtual ~CostFunction() {}
  // Ceres' interface: residuals and (nullable, per parameter block nullable) row-major Jacobians of ONE block on the host.
  // A probe for spot checks -- ceres::Solve never calls it, every block is evaluated by the gfx950 kernels.
  virtual bool Evaluate(double const *const *parameters, double *residuals, double **jacobians) const {
    (void)parameters; (void)residuals; (void)jacobians;
    return false;
  }
  // true if this block is an edge-alignment block; fills info
  virtual bool DescribeEdgeAlignmentBlock(EABlockInfo *) const { return false; }
  // non-NULL if this block is a ceres::NormalPrior
  virtual const NormalPrior *AsNormalPrior() const { return nullptr; }
};

// ---- minimal dense matrix / vector (ceres::Matrix, ceres::Vector are Eigen types in Ceres; these are enough to build a
// NormalPrior without Eigen -- NormalPrior also takes Eigen objects directly) ------------------------------------------
class Matrix {
 public:
  Matrix() : r_(0), c_(0) {}
  Matrix(int rows, int cols) : r_(rows), c_(cols), v_((size_t)rows * cols, 0.0) {}
  int rows() const { return r_; }
  int cols() const { return c_; }
  double &operator()(int i, int j) { return v_[(size_t)i * c_ + j]; }
  double operator()(int i, int j) const { return v_[(size_t)i * c_ + j]; }
  Matrix &setZero() { std::fill(v_.begin(), v_.end(), 0.0); return *this; }
  Matrix &setIdentity() {
    setZero();
    for (int i = 0; i < r_ && i < c_; ++i) (*this)(i, i) = 1.0;
    return *this;
  }
  const double *data() const { return v_.data(); }  // row-major
 private:
  int r_, c_;
  std::vector<double> v_;
};

class Vector {
 public:
  Vector() {}
  explicit Vector(int n) : v_((size_t)n, 0.0) {}
  int size() const { return (int)v_.size(); }
  double &operator()(int i) { return v_[(size_t)i]; }
  double operator()(int i) const { return v_[(size_t)i]; }
  double &operator[](int i) { return v_[(size_t)i]; }
  double operator[](int i) const { return v_[(size_t)i]; }
  Vector &setZero() { std::fill(v_.begin(), v_.end(), 0.0); return *this; }
  const double *data() const { return v_.data(); }
 private:
  std::vector<double> v_;
};

// ceres/normal_prior.h (Ceres <= 2.1): residual A (x - b) on ONE parameter block of size b.size(), A k x n.  Evaluate is the
// honest host computation (Jacobian = A, in the block's ambient coordinates); the solve folds the prior into the device's
// normal equations as H = A^T A (ea_problem_set_normal_prior).  Ceres takes a Matrix and a Vector; here anything with
// rows() / cols() / operator()(i, j) and size() / operator()(i) -- ceres::Matrix / Vector above, or Eigen types.
class NormalPrior : public CostFunction {
 public:
  template <typename MatrixT, typename VectorT>
  NormalPrior(const MatrixT &A, const VectorT &b) : k_((int)A.rows()), n_((int)A.cols()) {
    A_.resize((size_t)k_ * n_);
    b_.resize((size_t)b.size());
    for (int i = 0; i < k_; ++i)
      for (int j = 0; j < n_; ++j) A_[(size_t)i * n_ + j] = A(i, j);
    for (int j = 0; j < (int)b.size(); ++j) b_[(size_t)j] = b(j);
  }
  bool Evaluate(double const *const *parameters, double *residuals, double **jacobians) const override {
    if (!parameters || !parameters[0] || !residuals || (int)b_.size() != n_) return false;
    const double *x = parameters[0];
    for (int i = 0; i < k_; ++i) {
      double s = 0.0;
      for (int j = 0; j < n_; ++j) s += A_[(size_t)i * n_ + j] * (x[j] - b_[(size_t)j]);
      residuals[i] = s;
    }
    if (jacobians && jacobians[0]) std::copy(A_.begin(), A_.end(), jacobians[0]);
    return true;
  }
  const NormalPrior *AsNormalPrior() const override { return this; }
  int num_residuals() const { return k_; }
  int parameter_block_size() const { return (int)b_.size(); }
  const std::vector<double> &A() const { return A_; }  // k x n row-major
  const std::vector<double> &b() const { return b_; }
 private:
  int k_, n_;
  std::vector<double> A_, b_;
};

// AutoDiffCostFunction<Functor, 1, 4, 3>: owns the functor like Ceres does.  The functor must
// expose `bool ea_describe(ceres::EABlockInfo*) const` (edge_alignment_amd/include/EAResidue.h does).
template <typename Functor, int kNumResiduals, int N0 = 0, int N1 = 0, int N2 = 0>
class AutoDiffCostFunction : public CostFunction {
 public:
  explicit AutoDiffCostFunction(Functor *functor) : functor_(functor) {}
  // forward-mode differentiation of the functor's templated operator() with Jet<double, N0 + N1> (two parameter
  // blocks, as every cost function of the reference has: q[4], t[3])
  bool Evaluate(double const *const *parameters, double *residuals, double **jacobians) const override {
    static_assert(N2 == 0, "two parameter blocks");
    if (!jacobians) return (*functor_)(parameters[0], parameters[1], residuals);
    typedef Jet<double, N0 + N1> J;
    J p0[N0 > 0 ? N0 : 1], p1[N1 > 0 ? N1 : 1], r[kNumResiduals];
    for (int i = 0; i < N0; ++i) p0[i] = J(parameters[0][i], i);
    for (int i = 0; i < N1; ++i) p1[i] = J(parameters[1][i], N0 + i);
    if (!(*functor_)(p0, p1, r)) return false;
    for (int k = 0; k < kNumResiduals; ++k) {
      residuals[k] = r[k].a;
      if (jacobians[0]) for (int i = 0; i < N0; ++i) jacobians[0][k * N0 + i] = r[k].v[i];
      if (jacobians[1]) for (int i = 0; i < N1; ++i) jacobians[1][k * N1 + i] = r[k].v[N0 + i];
    }
    return true;
  }
  bool DescribeEdgeAlignmentBlock(EABlockInfo *info) const override {
    if (kNumResiduals != 1 || N0 != 4 || N1 != 3 || N2 != 0) return false;
    return functor_->ea_describe(info);
  }
  const Functor *functor() const { return functor_.get(); }

 private:
  std::unique_ptr<Functor> functor_;
};

// ---- local parameterisation -----------------------------------------------------------------
class LocalParameterization {
 public:
  virtual ~LocalParameterization() {}
  virtual bool Plus(const double *x, const double *delta, double *x_plus_delta) const = 0;
  virtual bool ComputeJacobian(const double *x, double *jacobian) const = 0;  // GlobalSize x LocalSize, row-major
  virtual int GlobalSize() const = 0;
  virtual int LocalSize() const = 0;
  virtual bool IsQuaternion() const { return false; }
  // non-NULL for a SubsetParameterization: constancy[i] != 0 = coordinate i held constant
  virtual const std::vector<char> *SubsetConstancy() const { return nullptr; }
};
// q+ = [cos|d|, sin|d|/|d| d] (x) q  — applied on the device by the LM-step kernel; the host forms below are Ceres'
// public definition (local_parameterization.cc), for callers that probe the parameterisation themselves
class QuaternionParameterization : public LocalParameterization {
 public:
  bool Plus(const double *x, const double *delta, double *x_plus_delta) const override {
    const double n = std::sqrt(delta[0] * delta[0] + delta[1] * delta[1] + delta[2] * delta[2]);
    if (n > 0.0) {
      const double s = std::sin(n) / n;
      const double d[4] = {std::cos(n), s * delta[0], s * delta[1], s * delta[2]};
      x_plus_delta[0] = d[0] * x[0] - d[1] * x[1] - d[2] * x[2] - d[3] * x[3];
      x_plus_delta[1] = d[0] * x[1] + d[1] * x[0] + d[2] * x[3] - d[3] * x[2];
      x_plus_delta[2] = d[0] * x[2] - d[1] * x[3] + d[2] * x[0] + d[3] * x[1];
      x_plus_delta[3] = d[0] * x[3] + d[1] * x[2] - d[2] * x[1] + d[3] * x[0];
    } else {
      for (int i = 0; i < 4; ++i) x_plus_delta[i] = x[i];
    }
    return true;
  }
  bool ComputeJacobian(const double *x, double *J) const override {
    J[0] = -x[1]; J[1] = -x[2]; J[2] = -x[3];
    J[3] = x[0];  J[4] = x[3];  J[5] = -x[2];
    J[6] = -x[3]; J[7] = x[0];  J[8] = x[1];
    J[9] = x[2];  J[10] = -x[1]; J[11] = x[0];
    return true;
  }
  int GlobalSize() const override { return 4; }
  int LocalSize() const override { return 3; }
  bool IsQuaternion() const override { return true; }
};

// ceres/local_parameterization.h (Ceres <= 2.1): the coordinates listed in constant_parameters are held, the others take
// the step.  The facade hosts it on the translation block (ea_problem_set_constant_parameters); on the quaternion block
// ceres::Solve reports it as unsupported.  The host forms are Ceres' definitions.
class SubsetParameterization : public LocalParameterization {
 public:
  SubsetParameterization(int size, const std::vector<int> &constant_parameters)
      : constancy_((size_t)(size > 0 ? size : 0), 0), local_size_(size > 0 ? size : 0) {
    for (int i : constant_parameters)
      if (i >= 0 && i < size && !constancy_[(size_t)i]) { constancy_[(size_t)i] = 1; --local_size_; }
  }
  bool Plus(const double *x, const double *delta, double *x_plus_delta) const override {
    for (size_t i = 0, j = 0; i < constancy_.size(); ++i) x_plus_delta[i] = constancy_[i] ? x[i] : x[i] + delta[j++];
    return true;
  }
  bool ComputeJacobian(const double *, double *jacobian) const override {  // GlobalSize x LocalSize, row-major
    for (size_t i = 0, j = 0; i < constancy_.size(); ++i) {
      for (int c = 0; c < local_size_; ++c) jacobian[i * (size_t)local_size_ + (size_t)c] = 0.0;
      if (!constancy_[i]) jacobian[i * (size_t)local_size_ + j++] = 1.0;
    }
    return true;
  }
  int GlobalSize() const override { return (int)constancy_.size(); }
  int LocalSize() const override { return local_size_; }
  const std::vector<char> *SubsetConstancy() const override { return &constancy_; }
 private:
  std::vector<char> constancy_;
  int local_size_;
};

// ---- problem --------------------------------------------------------------------------------
// ceres/crs_matrix.h: compressed-row sparse matrix as Problem::Evaluate hands it out
struct CRSMatrix {
  CRSMatrix() : num_rows(0), num_cols(0) {}
  int num_rows, num_cols;
  std::vector<int> cols, rows;
  std::vector<double> values;
};

class Problem {
 public:
  Problem() {}
  ~Problem() {
    for (auto *c : costs_) delete c;
    // a loss object may have been handed to several blocks (Ceres allows it): delete each once
    if (!std::is_sorted(losses_.begin(), losses_.end())) std::sort(losses_.begin(), losses_.end());
    losses_.erase(std::unique(losses_.begin(), losses_.end()), losses_.end());
    for (auto *l : losses_) delete l;
    for (auto *p : params_) delete p;
  }
  Problem(const Problem &) = delete;
  Problem &operator=(const Problem &) = delete;

  // standalone_edge_align.cpp:272  problem.AddResidualBlock(cost, new CauchyLoss(1.), q, t)
  void AddResidualBlock(CostFunction *cost, LossFunction *loss, double *q, double *t) {
    costs_.push_back(cost);
    if (loss && (losses_.empty() || losses_.back() != loss))
      losses_.push_back(loss);  // one `new CauchyLoss(1.)` per block in the reference; shared ones are fine too (~Problem)
    // What a block stores is its point and the index of its functor description: the reference adds one block per edge point
    // (44 457 per frame pair at stride 1), all describing the same functor; 64 bytes per block instead of the 430 of a full
    // description keep the list in cache while it is built and gathered (see profiles/r02_facade_timing.txt).
    EABlockInfo info;
    Block b;
    b.ok = cost->DescribeEdgeAlignmentBlock(&info);
    b.X = info.X; b.Y = info.Y; b.Z = info.Z;
    b.fam = -1;
    if (b.ok) {
      if (last_fam_ >= 0 && SameFunctor(fams_[(size_t)last_fam_], info)) b.fam = last_fam_;
      else {
        for (size_t k = 0; k < fams_.size() && b.fam < 0; ++k)
          if (SameFunctor(fams_[k], info)) b.fam = (int)k;
        if (b.fam < 0) { fams_.push_back(info); b.fam = (int)fams_.size() - 1; }
        last_fam_ = b.fam;
      }
    }
    b.loss = loss;
    b.q = q;
    b.t = t;
    blocks_.push_back(b);
  }
  // ceres::NormalPrior on one parameter block: problem.AddResidualBlock(new NormalPrior(A, b), NULL, x).  The facade hosts
  // NormalPriors on the pose the EAResidue blocks share, without a loss, at most one per block (ProblemAccess::Build);
  // any other single-block cost function is kept and refused there.
  void AddResidualBlock(CostFunction *cost, LossFunction *loss, double *x) {
    costs_.push_back(cost);
    if (loss && (losses_.empty() || losses_.back() != loss)) losses_.push_back(loss);
    priors_.push_back(PriorBlock{cost, loss, x, blocks_.size()});
  }
  // standalone_edge_align.cpp:277-278
  void SetParameterization(double *values, LocalParameterization *p) {
    params_.push_back(p);
    if (p && p->IsQuaternion()) quat_param_on_ = values;
    // the last parameterization set on a block holds: a later non-subset one takes the block's held coordinates back
    for (size_t i = 0; i < subsets_.size(); ++i)
      if (subsets_[i].first == values) { subsets_.erase(subsets_.begin() + (long)i); break; }
    if (p && p->SubsetConstancy()) subsets_.push_back(std::make_pair(values, (const LocalParameterization *)p));
  }
  // Parameter blocks are added by AddResidualBlock; these exist for code that names them first.  `size` is not recorded: the
  // block sizes are those of the EAResidue blocks (4, 3), and Build checks a SubsetParameterization's size against them.
  void AddParameterBlock(double *, int) {}
  void AddParameterBlock(double *values, int, LocalParameterization *p) { SetParameterization(values, p); }
  // A constant block is removed from the program: ceres::Solve leaves it bit for bit as it is and ceres::Covariance returns
  // zero blocks for it (ea_problem_set_constant_parameters).  Problem::Evaluate is not affected.
  void SetParameterBlockConstant(double *values) {
    if (!IsParameterBlockConstant(values)) constant_.push_back(values);
  }
  void SetParameterBlockVariable(double *values) {
    constant_.erase(std::remove(constant_.begin(), constant_.end(), values), constant_.end());
  }
  bool IsParameterBlockConstant(double *values) const {
    return std::find(constant_.begin(), constant_.end(), values) != constant_.end();
  }
  int NumResidualBlocks() const { return (int)(blocks_.size() + priors_.size()); }
  int NumResiduals() const {
    int n = (int)blocks_.size();
    for (const auto &pb : priors_) n += pb.cost->AsNormalPrior() ? pb.cost->AsNormalPrior()->num_residuals() : 0;
    return n;
  }
  int NumParameterBlocks() const { return blocks_.empty() ? 0 : 2; }  // the quaternion and the translation
  int NumParameters() const { return blocks_.empty() ? 0 : 7; }

  // src/SolveEA.cpp:241  problem.Evaluate(Problem::EvaluateOptions(), &cost, &residuals, NULL, NULL)
  // cost = 1/2 sum rho(r^2); residuals: one per block in the order they were added (k per NormalPrior block), loss-corrected like
  // Ceres' apply_loss_function = true; gradient: the 6 tangent-space entries (J^T r); jacobian: one row per block in the same
  // order, six columns [d r / d delta (3) | d r / d t (3)] -- the parameter blocks' local sizes in the order
  // AddResidualBlock names them (quaternion, translation) -- as a compressed-row matrix with dense rows.
  struct EvaluateOptions {
    bool apply_loss_function = true;
    int ea_dtype = EA_F64;
    int ea_device = 0;
  };
  inline bool Evaluate(const EvaluateOptions &opt, double *cost, std::vector<double> *residuals,
                       std::vector<double> *gradient, CRSMatrix *jacobian);

 private:
  struct Block {
    double X, Y, Z;
    int fam;   // index into fams_: everything of the functor's description but the point
    bool ok;
    LossFunction *loss;
    double *q, *t;
  };
  static bool SameFunctor(const EABlockInfo &x, const EABlockInfo &y) {
    if (x.grid_data != y.grid_data || x.grid_rows != y.grid_rows || x.grid_cols != y.grid_cols) return false;
    if (x.fx != y.fx || x.fy != y.fy || x.cx != y.cx || x.cy != y.cy) return false;
    if (x.z_guard != y.z_guard || x.z_eps != y.z_eps || x.rot_transposed != y.rot_transposed) return false;
    if (x.variant != y.variant) return false;
    if (x.variant & 1)
      for (int i = 0; i < 5; ++i) if (x.dist[i] != y.dist[i]) return false;
    if (x.variant & 2)
      for (int i = 0; i < 16; ++i) if (x.T12[i] != y.T12[i] || x.T12inv[i] != y.T12inv[i]) return false;
    return true;
  }
  // a single-block residual (NormalPrior): `before` = EAResidue blocks added ahead of it (its place in block order)
  struct PriorBlock {
    CostFunction *cost;
    LossFunction *loss;
    double *x;
    size_t before;
  };
  std::vector<Block> blocks_;
  std::vector<PriorBlock> priors_;
  std::vector<EABlockInfo> fams_;   // distinct functor descriptions (X, Y, Z of the entry unused)
  int last_fam_ = -1;
  std::vector<CostFunction *> costs_;
  std::vector<LossFunction *> losses_;
  std::vector<LocalParameterization *> params_;
  double *quat_param_on_ = nullptr;
  std::vector<double *> constant_;                                          // SetParameterBlockConstant
  std::vector<std::pair<double *, const LocalParameterization *>> subsets_;  // SubsetParameterization per block
  friend class ProblemAccess;
};

// ---- solver ---------------------------------------------------------------------------------
struct Solver {
  struct Options {
    MinimizerType minimizer_type = TRUST_REGION;
    TrustRegionStrategyType trust_region_strategy_type = LEVENBERG_MARQUARDT;
    DoglegType dogleg_type = TRADITIONAL_DOGLEG;
    LinearSolverType linear_solver_type = DENSE_QR;  // accepted; the 6x6 system is solved on the device
    int max_num_iterations = 50;
    double max_solver_time_in_seconds = 1e9;
    int num_threads = 1;
    double initial_trust_region_radius = 1e4;
    double max_trust_region_radius = 1e16;
    double min_trust_region_radius = 1e-32;
    double min_relative_decrease = 1e-3;
    double min_lm_diagonal = 1e-6;
    double max_lm_diagonal = 1e32;
    int max_num_consecutive_invalid_steps = 5;
    double function_tolerance = 1e-6;
    double gradient_tolerance = 1e-10;
    double parameter_tolerance = 1e-8;
    bool jacobi_scaling = true;
    bool minimizer_progress_to_stdout = false;
    // not part of Ceres: arithmetic type of the per-point evaluation and the GPU to use
    int ea_dtype = EA_F64;
    int ea_device = 0;
  };
  struct Summary {
    TerminationType termination_type = FAILURE;
    std::string message = "ceres::Solve was not called.";
    double initial_cost = -1, final_cost = -1;
    int num_successful_steps = -1, num_unsuccessful_steps = -1;
    int num_residual_blocks = 0, num_residuals = 0;
    int num_parameter_blocks = 2, num_parameters = 7, num_effective_parameters = 6;
    // the program Solve ran after constant blocks and constant coordinates were removed (blocks, ambient and tangent sizes)
    int num_parameter_blocks_reduced = 2, num_parameters_reduced = 7, num_effective_parameters_reduced = 6;
    double total_time_in_seconds = -1;
    int ea_num_gpu_problems = 0;  // not part of Ceres: the GPU problems Solve built (one per residual family)
    ea_summary detail{};

    bool IsSolutionUsable() const { return termination_type == CONVERGENCE || termination_type == NO_CONVERGENCE; }
    std::string BriefReport() const {
      std::ostringstream o;
      o << "edge_alignment_amd Report: Iterations: " << (num_successful_steps + num_unsuccessful_steps)
        << ", Initial cost: " << initial_cost << ", Final cost: " << final_cost
        << ", Termination: " << TermName();
      return o.str();
    }
    std::string FullReport() const {
      char buf[2048];
      std::snprintf(buf, sizeof(buf),
                    "\nSolver Summary (edge_alignment_amd, MI355X gfx950; ceres:: facade)\n\n"
                    "                                     Original                  Reduced\n"
                    "Parameter blocks %26d %24d\nParameters %32d %24d\nEffective parameters %22d %24d\n"
                    "Residual blocks %27d\nResidual %34d\n\n"
                    "Minimizer                        TRUST_REGION\n"
                    "Linear solver          6x6 normal equations (device)\n\n"
                    "Cost:\nInitial %35.6e\nFinal %37.6e\nChange %36.6e\n\n"
                    "Minimizer iterations %22d\nSuccessful steps %26d\nUnsuccessful steps %24d\n\n"
                    "Time (in seconds):\nTotal %37.4f\n\nTermination: %28s (%s)\n",
                    num_parameter_blocks, num_parameter_blocks_reduced, num_parameters, num_parameters_reduced,
                    num_effective_parameters, num_effective_parameters_reduced, num_residual_blocks,
                    num_residuals, initial_cost, final_cost, initial_cost - final_cost,
                    num_successful_steps + num_unsuccessful_steps, num_successful_steps, num_unsuccessful_steps,
                    total_time_in_seconds, TermName(), message.c_str());
      return std::string(buf);
    }
    const char *TermName() const {
      switch (termination_type) {
        case CONVERGENCE: return "CONVERGENCE";
        case NO_CONVERGENCE: return "NO_CONVERGENCE";
        case FAILURE: return "FAILURE";
        default: return "USER";
      }
    }
  };
};

namespace internal {
inline const char *WhyMessage(int why) {
  switch (why) {
    case EA_WHY_FUNCTION_TOL: return "Function tolerance reached.";
    case EA_WHY_GRADIENT_TOL: return "Gradient tolerance reached.";
    case EA_WHY_PARAMETER_TOL: return "Parameter tolerance reached.";
    case EA_WHY_MAX_ITERATIONS: return "Maximum number of iterations reached.";
    case EA_WHY_MIN_RADIUS: return "Minimum trust region radius reached.";
    case EA_WHY_INITIAL_EVAL_FAILED: return "Initial residual and Jacobian evaluation failed.";
    case EA_WHY_TOO_MANY_INVALID_STEPS: return "Number of consecutive invalid steps more than Solver::Options::max_num_consecutive_invalid_steps.";
    case EA_WHY_EVAL_FAILED: return "Residual and Jacobian evaluation failed.";
    default: return "";
  }
}
}  // namespace internal

// standalone_edge_align.cpp:286  ceres::Solve(options, &problem, &summary)
inline void Solve(const Solver::Options &options, Problem *problem, Solver::Summary *summary);

class ProblemAccess {  // keeps Problem's internals private to user code
 public:
  // A residual family: the blocks that share interpolator, intrinsics, functor variant and loss (kind and scale; a
  // ScaledLoss factor is the block's weight, so N blocks with N different factors are still one family).  weights[j] = factor
  // of the family's j-th block, in the order the blocks were added; weighted = some factor differs from 1.
  struct Family { const Problem::Block *first; std::vector<double> xyz; std::vector<int> idx; std::vector<double> weights; bool weighted; };
  // the grouping Build uploads, on the host alone (no device is touched); false with *err set
  static bool Families(const Problem *problem, std::vector<Family> *fams_out, std::string *err) {
    const auto &blocks = problem->blocks_;
    std::vector<Family> &fams = *fams_out;
    fams.clear();
    if (blocks.empty()) { *err = "a NormalPrior needs EAResidue blocks on the same pose (a problem of priors only cannot be hosted)"; return false; }
    const auto &b0 = blocks[0];
    for (size_t i = 0; i < blocks.size(); ++i) {
      const auto &b = blocks[i];
      if (!b.ok) { *err = "residual block is not an EAResidue-family block (this facade only hosts the edge-alignment hot path)"; return false; }
      if (b.q != b0.q || b.t != b0.t) { *err = "all residual blocks must share one (quaternion, translation) pair"; return false; }
      Family *f = nullptr;
      for (auto &cand : fams)
        if (SameFamily(*cand.first, b)) { f = &cand; break; }
      if (!f) {
        fams.push_back(Family{&b, {}, {}, {}, false});
        f = &fams.back();
        f->xyz.reserve(3 * (blocks.size() - i));  // (usually the one family: no regrowth while 44 457 blocks are gathered)
        f->idx.reserve(blocks.size() - i);
      }
      f->xyz.push_back(b.X); f->xyz.push_back(b.Y); f->xyz.push_back(b.Z);
      f->idx.push_back((int)i);
      const double w = b.loss ? b.loss->ea_weight() : 1.0;
      if (!(w >= 0.0) || !(w <= 1.7976931348623157e308)) { *err = "ScaledLoss: the scale of a residual block's loss must be finite and >= 0"; return false; }
      f->weights.push_back(w);
      f->weighted = f->weighted || w != 1.0;
    }
    return true;
  }

  // Blocks -> residual families (same interpolator, intrinsics, functor variant and loss) -> one GPU problem per
  // family, the first one carrying the others as terms: all of them share (q, t), the way the reference adds
  // camera-1 and camera-2 blocks to one ceres::Problem (standalone_edge_align.cpp:791-803).  order[k] = indices of
  // family k's blocks in the order they were added.  Returns EA_OK, a libea_hip error code, or -1000 with *err set
  // for a problem this facade cannot host.
  static int Build(Problem *problem, int dtype, int device, std::vector<ea_problem *> *ps_out,
                   std::vector<std::vector<int>> *order, std::string *err, int *held_out = nullptr) {
    const auto &blocks = problem->blocks_;
    std::vector<Family> fams;
    if (!Families(problem, &fams, err)) return -1000;
    const auto &b0 = blocks[0];
    if (problem->quat_param_on_ != b0.q) { *err = "the quaternion block needs QuaternionParameterization (problem.SetParameterization)"; return -1000; }
    const NormalPrior *prior_on[2] = {nullptr, nullptr};  // (q, t)
    for (const auto &pb : problem->priors_) {
      const NormalPrior *np = pb.cost->AsNormalPrior();
      if (!np) { *err = "single-block residual is not a NormalPrior (this facade only hosts NormalPriors beside the EAResidue blocks)"; return -1000; }
      if (pb.loss) { *err = "a NormalPrior block cannot take a loss function"; return -1000; }
      const int blk = pb.x == b0.q ? 0 : (pb.x == b0.t ? 1 : -1);
      if (blk < 0) { *err = "a NormalPrior must sit on the (quaternion, translation) pair the EAResidue blocks share"; return -1000; }
      if (np->parameter_block_size() != (blk == 0 ? 4 : 3) || (int)np->A().size() != np->num_residuals() * (blk == 0 ? 4 : 3) ||
          np->num_residuals() < 1) {
        *err = "NormalPrior size does not match its parameter block (A k x 4 on the quaternion, k x 3 on the translation)"; return -1000;
      }
      if (prior_on[blk]) { *err = "at most one NormalPrior per parameter block"; return -1000; }
      prior_on[blk] = np;
    }
    int held[6];
    if (!ConstantMask(problem, held, err)) return -1000;
    if (held_out)  // (the mask the problem was built with: ceres::Solve derives the summary's reduced counts from it)
      for (int i = 0; i < 6; ++i) held_out[i] = held[i];
    std::vector<ea_problem *> &ps = *ps_out;
    ps.assign(fams.size(), nullptr);
    order->clear();
    int rc = EA_OK;
    for (size_t k = 0; k < fams.size() && rc == EA_OK; ++k) {
      const EABlockInfo &bi = problem->fams_[(size_t)fams[k].first->fam];
      order->push_back(fams[k].idx);
      ea_camera cam = {bi.fx, bi.fy, bi.cx, bi.cy};
      rc = ea_problem_create(&ps[k], &cam, dtype, device);
      if (rc == EA_OK) rc = ea_problem_set_points(ps[k], fams[k].xyz.data(), (int64_t)(fams[k].xyz.size() / 3), 3);
      if (rc == EA_OK) rc = ea_problem_set_dt(ps[k], bi.grid_data, bi.grid_rows, bi.grid_cols);
      if (rc == EA_OK) rc = ea_problem_set_flavour(ps[k], bi.z_guard, bi.z_eps, bi.rot_transposed);
      if (rc == EA_OK && (bi.variant & 1)) rc = ea_problem_set_distortion(ps[k], bi.dist[0], bi.dist[1], bi.dist[2], bi.dist[3], bi.dist[4]);
      if (rc == EA_OK && (bi.variant & 2)) rc = ea_problem_set_second_camera(ps[k], bi.T12, bi.T12inv);
      if (rc == EA_OK) {
        int kind = EA_LOSS_TRIVIAL; double a = 1.0;
        if (fams[k].first->loss) { kind = fams[k].first->loss->ea_kind(); a = fams[k].first->loss->ea_scale(); }
        rc = ea_problem_set_loss(ps[k], kind, a);
      }
      if (rc == EA_OK && fams[k].weighted)  // ScaledLoss factors: the family's per-point weights, in block order
        rc = ea_problem_set_weights(ps[k], fams[k].weights.data(), (int64_t)fams[k].weights.size());
      if (rc == EA_OK && k > 0) rc = ea_problem_add_term(ps[0], ps[k]);
    }
    if (rc == EA_OK && (held[0] | held[1] | held[2] | held[3] | held[4] | held[5]))  // the mask too goes on the head problem
      rc = ea_problem_set_constant_parameters(ps[0], held);
    for (int blk = 0; blk < 2 && rc == EA_OK; ++blk)  // the priors go on the head problem: every term shares its pose
      if (prior_on[blk])
        rc = ea_problem_set_normal_prior(ps[0], blk, prior_on[blk]->A().data(), prior_on[blk]->num_residuals(),
                                         prior_on[blk]->b().data());
    return rc;
  }

  // SetParameterBlockConstant / SubsetParameterization -> the tangent mask of ea_problem_set_constant_parameters
  // ([delta(3) | t(3)]); false with *err set for what the facade cannot host
  static bool ConstantMask(const Problem *problem, int held[6], std::string *err) {
    for (int i = 0; i < 6; ++i) held[i] = 0;
    if (problem->blocks_.empty()) return true;
    double *q = problem->blocks_[0].q, *t = problem->blocks_[0].t;
    for (const auto &sb : problem->subsets_) {
      if (sb.first == q) { *err = "SubsetParameterization on the quaternion block is not supported (SetParameterBlockConstant holds all of it)"; return false; }
      if (sb.first != t) { *err = "a SubsetParameterization must sit on the translation block the EAResidue blocks share"; return false; }
      const std::vector<char> &c = *sb.second->SubsetConstancy();
      if (c.size() != 3) { *err = "SubsetParameterization size does not match the translation block (3)"; return false; }
      for (int i = 0; i < 3; ++i) held[3 + i] = c[(size_t)i] ? 1 : 0;
    }
    for (double *cb : problem->constant_) {
      if (cb == q) held[0] = held[1] = held[2] = 1;
      else if (cb == t) held[3] = held[4] = held[5] = 1;
      else { *err = "SetParameterBlockConstant names a block that is not the (quaternion, translation) pair of the EAResidue blocks"; return false; }
    }
    return true;
  }

  // the (quaternion, translation) pair every block of the problem shares; false for an empty problem
  static bool PoseBlocks(const Problem *problem, double **q, double **t) {
    if (problem->blocks_.empty()) return false;
    *q = problem->blocks_[0].q;
    *t = problem->blocks_[0].t;
    return true;
  }

  static bool Evaluate(Problem *problem, const Problem::EvaluateOptions &opt, double *cost, std::vector<double> *residuals,
                       std::vector<double> *gradient, CRSMatrix *jacobian) {
    const auto &blocks = problem->blocks_;
    const auto &priors = problem->priors_;
    // rows in block order: EAResidue block i sits behind the rows of every prior added before it
    const size_t nrows = (size_t)problem->NumResiduals();
    std::vector<size_t> row_of(blocks.size()), prior_row(priors.size());
    {
      size_t row = 0, j = 0;
      for (size_t i = 0; i <= blocks.size(); ++i) {
        for (; j < priors.size() && priors[j].before == i; ++j) {
          prior_row[j] = row;
          row += priors[j].cost->AsNormalPrior() ? (size_t)priors[j].cost->AsNormalPrior()->num_residuals() : 0;
        }
        if (i < blocks.size()) row_of[i] = row++;
      }
    }
    if (jacobian) {
      jacobian->num_rows = (int)nrows;
      jacobian->num_cols = blocks.empty() ? 0 : 6;
      jacobian->rows.assign(nrows + 1, 0);
      jacobian->cols.assign(nrows * 6, 0);
      jacobian->values.assign(nrows * 6, 0.0);
      for (size_t i = 0; i < nrows; ++i) {
        jacobian->rows[i + 1] = (int)(6 * (i + 1));
        for (int a = 0; a < 6; ++a) jacobian->cols[6 * i + a] = a;
      }
    }
    if (blocks.empty() && priors.empty()) {
      if (cost) *cost = 0.0;
      if (residuals) residuals->clear();
      if (gradient) gradient->clear();
      return true;
    }
    std::vector<ea_problem *> ps;
    std::vector<std::vector<int>> order;
    std::string err;
    int rc = Build(problem, opt.ea_dtype, opt.ea_device, &ps, &order, &err);
    if (rc != EA_OK) {  // (nothing was created; a problem of priors only has no blocks[0] to read the pose from)
      for (auto *p : ps)
        if (p) ea_problem_destroy(p);
      return false;
    }
    const double *q = blocks[0].q, *t = blocks[0].t;
    double c = 0.0, JtJ[36], Jtr[6];
    int64_t bad = 0;
    if (rc == EA_OK) rc = ea_eval(ps[0], q, t, &c, JtJ, Jtr, &bad);  // the problem with all its terms
    if (rc == EA_OK && (residuals || jacobian)) {
      if (residuals) residuals->assign(nrows, 0.0);
      for (size_t k = 0; k < ps.size() && rc == EA_OK; ++k) {
        std::vector<double> r(order[k].size()), J(jacobian ? order[k].size() * 6 : 0);
        // a term evaluated on its own: its residuals (and 1x6 rows) in the order its blocks were added
        rc = ea_eval_points(ps[k], q, t, r.data(), jacobian ? J.data() : nullptr, opt.apply_loss_function ? 1 : 0);
        for (size_t i = 0; i < r.size(); ++i) {
          const size_t row = row_of[(size_t)order[k][i]];
          if (residuals) (*residuals)[row] = r[i];
          if (jacobian)
            for (int a = 0; a < 6; ++a) jacobian->values[6 * row + a] = J[6 * i + a];
        }
      }
      // the NormalPriors' rows on the host: r = A (x - b), tangent Jacobian A P(q) on the quaternion, A on the translation
      for (size_t j = 0; j < priors.size(); ++j) {
        const NormalPrior *np = priors[j].cost->AsNormalPrior();
        const int k = np->num_residuals(), n = np->parameter_block_size();
        std::vector<double> r((size_t)k), A((size_t)k * n);
        const double *x = priors[j].x;
        double *jac[1] = {A.data()};
        np->Evaluate(&x, r.data(), jac);
        const bool on_q = priors[j].x == q;
        double P[12];
        if (on_q) QuaternionParameterization().ComputeJacobian(q, P);
        for (int i = 0; i < k; ++i) {
          const size_t row = prior_row[j] + (size_t)i;
          if (residuals) (*residuals)[row] = r[(size_t)i];
          if (!jacobian) continue;
          for (int a = 0; a < 3; ++a) {
            double v = 0.0;
            if (on_q)
              for (int m = 0; m < 4; ++m) v += A[(size_t)i * 4 + m] * P[3 * m + a];
            else
              v = A[(size_t)i * 3 + a];
            jacobian->values[6 * row + (on_q ? 0 : 3) + a] = v;
          }
        }
      }
    }
    for (auto *p : ps)
      if (p) ea_problem_destroy(p);
    if (rc != EA_OK || bad > 0) return false;  // Ceres: a failed residual block fails the evaluation
    if (cost) *cost = c;
    if (gradient) gradient->assign(Jtr, Jtr + 6);
    return true;
  }

  static void Run(const Solver::Options &options, Problem *problem, Solver::Summary *summary) {
    Solver::Summary &s = *summary;
    s = Solver::Summary();
    const auto &blocks = problem->blocks_;
    s.num_residual_blocks = problem->NumResidualBlocks();
    s.num_residuals = problem->NumResiduals();
    auto fail = [&](const std::string &m) { s.termination_type = FAILURE; s.message = m; };
    if (options.minimizer_type != TRUST_REGION) return fail("only TRUST_REGION is supported");
    if (blocks.empty() && problem->priors_.empty()) { s.termination_type = CONVERGENCE; s.message = "No residual blocks."; s.initial_cost = s.final_cost = 0; s.num_successful_steps = s.num_unsuccessful_steps = 0; return; }
    std::vector<ea_problem *> ps;
    std::vector<std::vector<int>> order;
    std::string berr;
    int held[6] = {0, 0, 0, 0, 0, 0};
    int rc = Build(problem, options.ea_dtype, options.ea_device, &ps, &order, &berr, held);
    if (rc == -1000) return fail(berr);
    int built = 0;
    for (const ea_problem *p : ps) built += p ? 1 : 0;
    const auto &b0 = blocks[0];  // (Build refused a problem without EAResidue blocks)
    {
      const int free_q = 3 - held[0] - held[1] - held[2], free_t = 3 - held[3] - held[4] - held[5];
      s.num_parameter_blocks_reduced = (free_q > 0) + (free_t > 0);
      s.num_parameters_reduced = (free_q > 0 ? 4 : 0) + (free_t > 0 ? 3 : 0);
      s.num_effective_parameters_reduced = free_q + free_t;
    }
    ea_options o;
    ea_default_options(&o);
    o.max_num_iterations = options.max_num_iterations;
    o.function_tolerance = options.function_tolerance;
    o.gradient_tolerance = options.gradient_tolerance;
    o.parameter_tolerance = options.parameter_tolerance;
    o.initial_trust_region_radius = options.initial_trust_region_radius;
    o.max_trust_region_radius = options.max_trust_region_radius;
    o.min_trust_region_radius = options.min_trust_region_radius;
    o.min_relative_decrease = options.min_relative_decrease;
    o.min_lm_diagonal = options.min_lm_diagonal;
    o.max_lm_diagonal = options.max_lm_diagonal;
    o.max_num_consecutive_invalid_steps = options.max_num_consecutive_invalid_steps;
    o.jacobi_scaling = options.jacobi_scaling ? 1 : 0;
    o.strategy = options.trust_region_strategy_type == DOGLEG ? EA_STRATEGY_DOGLEG : EA_STRATEGY_LM;
    o.minimizer_progress_to_stdout = options.minimizer_progress_to_stdout ? 1 : 0;
    if (rc == EA_OK) rc = ea_solve(ps[0], &o, b0.q, b0.t, &s.detail);  // q, t updated in place, like Ceres
    const std::string err = rc != EA_OK ? std::string(ea_last_error()) : std::string();
    for (size_t k = 0; k < ps.size(); ++k)
      if (ps[k]) ea_problem_destroy(ps[k]);
    if (rc != EA_OK) return fail(std::string("libea_hip: ") + err);
    s.termination_type = s.detail.termination == EA_CONVERGENCE ? CONVERGENCE : (s.detail.termination == EA_NO_CONVERGENCE ? NO_CONVERGENCE : FAILURE);
    s.message = internal::WhyMessage(s.detail.why);
    s.initial_cost = s.detail.initial_cost;
    s.final_cost = s.detail.final_cost;
    s.num_successful_steps = s.detail.num_successful_steps;
    s.num_unsuccessful_steps = s.detail.num_unsuccessful_steps;
    s.total_time_in_seconds = s.detail.total_time_ms * 1e-3;
    s.ea_num_gpu_problems = built;
  }

 private:
  // same functor description (by construction: same index) and an equivalent loss -- up to a ScaledLoss factor, which is
  // the block's weight and not part of the family
  static bool SameFamily(const Problem::Block &a, const Problem::Block &b) {
    return a.fam == b.fam && (a.loss == b.loss || SameLoss(a.loss, b.loss));
  }
  static bool SameLoss(const LossFunction *a, const LossFunction *b) {
    const int ka = a ? a->ea_kind() : EA_LOSS_TRIVIAL, kb = b ? b->ea_kind() : EA_LOSS_TRIVIAL;
    if (ka != kb) return false;
    if (ka == EA_LOSS_TRIVIAL) return true;
    return a->ea_scale() == b->ea_scale();
  }
};

inline bool Problem::Evaluate(const EvaluateOptions &opt, double *cost, std::vector<double> *residuals,
                              std::vector<double> *gradient, CRSMatrix *jacobian) {
  return ProblemAccess::Evaluate(this, opt, cost, residuals, gradient, jacobian);
}

inline void Solve(const Solver::Options &options, Problem *problem, Solver::Summary *summary) {
  ProblemAccess::Run(options, problem, summary);
}

}  // namespace ceres

#include "covariance.h"
