// ceres::NormalPrior beside the EAResidue blocks of the reference's test1 problem: a prior on t (and, with argv[3] = 1, one
// on q), the way a motion model or an odometry translation enters a Ceres problem.  Input: the problem file of
// examples/standalone_test1.cpp; prints the solved pose, Problem::Evaluate's residual count and gradient as one line of
// numbers each.  Compiled -std=c++14 -Wall -Werror, with the facade's ceres::Matrix / Vector or (-DEA_EIGEN_LIKE) a small
// stand-in with Eigen's element access.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "EAResidue.h"
#include "ceres/ceres.h"

#ifdef EA_EIGEN_LIKE
// what NormalPrior needs of an Eigen::MatrixXd / Eigen::VectorXd: rows(), cols(), operator()(i, j); size(), operator()(i)
struct DenseM {
  DenseM(int r, int c) : r_(r), c_(c), v_((size_t)r * c, 0.0) {}
  long rows() const { return r_; }
  long cols() const { return c_; }
  double &operator()(long i, long j) { return v_[(size_t)(i * c_ + j)]; }
  double operator()(long i, long j) const { return v_[(size_t)(i * c_ + j)]; }
  int r_, c_;
  std::vector<double> v_;
};
struct DenseV {
  explicit DenseV(int n) : v_((size_t)n, 0.0) {}
  long size() const { return (long)v_.size(); }
  double &operator()(long i) { return v_[(size_t)i]; }
  double operator()(long i) const { return v_[(size_t)i]; }
  std::vector<double> v_;
};
typedef DenseM Mat;
typedef DenseV Vec;
static void identity(Mat &A, double s) { for (long i = 0; i < A.rows() && i < A.cols(); ++i) A(i, i) = s; }
#else
typedef ceres::Matrix Mat;
typedef ceres::Vector Vec;
static void identity(Mat &A, double s) {
  A.setIdentity();
  for (int i = 0; i < A.rows() && i < A.cols(); ++i) A(i, i) = s;
}
#endif

static void print(const char *name, const double *v, int n) {
  std::printf("%s", name);
  for (int i = 0; i < n; ++i) std::printf(" %.17g", v[i]);
  std::printf("\n");
}

int main(int argc, char **argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s problem.bin [stride] [prior_on_q]\n", argv[0]); return 2; }
  const int stride = argc > 2 ? std::atoi(argv[2]) : 30;
  const bool on_q = argc > 3 && std::atoi(argv[3]) != 0;
  std::FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t N, rows, cols;
  double fx, fy, cx, cy;
  if (std::fread(&N, 4, 1, f) != 1 || std::fread(&rows, 4, 1, f) != 1 || std::fread(&cols, 4, 1, f) != 1) return 2;
  if (std::fread(&fx, 8, 1, f) != 1 || std::fread(&fy, 8, 1, f) != 1 || std::fread(&cx, 8, 1, f) != 1 || std::fread(&cy, 8, 1, f) != 1) return 2;
  std::vector<double> a_X(4 * (size_t)N), e_disTrans((size_t)rows * cols);
  if (std::fread(a_X.data(), 8, a_X.size(), f) != a_X.size()) return 2;
  if (std::fread(e_disTrans.data(), 8, e_disTrans.size(), f) != e_disTrans.size()) return 2;
  std::fclose(f);

  ceres::Grid2D<double, 1> grid(e_disTrans.data(), 0, cols, 0, rows);
  ceres::BiCubicInterpolator<ceres::Grid2D<double, 1>> interp(grid);
  double q[4] = {1, 0, 0, 0}, t[3] = {0, 0, 0};
  ceres::Problem problem;
  int nea = 0;
  for (int i = 0; i < N; i += stride, ++nea)
    problem.AddResidualBlock(EAResidue::Create(fx, fy, cx, cy, a_X[4 * (size_t)i], a_X[4 * (size_t)i + 1], a_X[4 * (size_t)i + 2], interp),
                             new ceres::CauchyLoss(1.), q, t);
  Mat At(3, 3);
  identity(At, 20.0);
  Vec bt(3);
  bt(0) = 0.01; bt(1) = -0.02; bt(2) = 0.005;
  problem.AddResidualBlock(new ceres::NormalPrior(At, bt), NULL, t);
  if (on_q) {
    Mat Aq(4, 4);
    identity(Aq, 50.0);
    Vec bq(4);
    bq(0) = 1.0;
    problem.AddResidualBlock(new ceres::NormalPrior(Aq, bq), NULL, q);
  }
  problem.SetParameterization(q, new ceres::QuaternionParameterization);
  ceres::Solver::Options options;
  ceres::Solver::Summary summary;
  ceres::Solve(options, &problem, &summary);
  if (summary.termination_type == ceres::FAILURE) { std::printf("solve failed: %s\n", summary.message.c_str()); return 1; }
  double cost = 0.0;
  std::vector<double> residuals, gradient;
  ceres::CRSMatrix jacobian;
  if (!problem.Evaluate(ceres::Problem::EvaluateOptions(), &cost, &residuals, &gradient, &jacobian)) {
    std::printf("evaluate failed\n");
    return 1;
  }
  const double counts[4] = {(double)nea, (double)residuals.size(), (double)jacobian.num_rows, (double)problem.NumResiduals()};
  print("q", q, 4);
  print("t", t, 3);
  print("counts", counts, 4);
  print("cost", &cost, 1);
  print("gradient", gradient.data(), (int)gradient.size());
  print("prior_rows", residuals.data() + nea, (int)residuals.size() - nea);
  print("prior_jacobian", jacobian.values.data() + 6 * (size_t)nea, 6 * ((int)residuals.size() - nea));  // (block order: t, then q)
  return 0;
}
