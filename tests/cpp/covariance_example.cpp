// ceres::Covariance the way the Ceres documentation uses it, right after ceres::Solve, on the reference's test1 problem
// (standalone_edge_align.cpp:256-293 set-up).  Input: the problem file of examples/standalone_test1.cpp; prints the pose
// and the ambient and tangent blocks as one line of numbers each.  Compiled -std=c++14 -Wall -Werror.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "EAResidue.h"
#include "ceres/ceres.h"

using ceres::CauchyLoss;

static void print(const char *name, const double *v, int n) {
  std::printf("%s", name);
  for (int i = 0; i < n; ++i) std::printf(" %.17g", v[i]);
  std::printf("\n");
}

int main(int argc, char **argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s problem.bin [stride]\n", argv[0]); return 2; }
  const int stride = argc > 2 ? std::atoi(argv[2]) : 30;
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
  for (int i = 0; i < N; i += stride)
    problem.AddResidualBlock(EAResidue::Create(fx, fy, cx, cy, a_X[4 * (size_t)i], a_X[4 * (size_t)i + 1], a_X[4 * (size_t)i + 2], interp),
                             new CauchyLoss(1.), q, t);
  problem.SetParameterization(q, new ceres::QuaternionParameterization);
  ceres::Solver::Options options;
  ceres::Solver::Summary summary;
  ceres::Solve(options, &problem, &summary);

  ceres::Covariance::Options cov_options;
  ceres::Covariance covariance(cov_options);
  std::vector<std::pair<const double *, const double *>> covariance_blocks;
  covariance_blocks.push_back(std::make_pair(q, q));
  covariance_blocks.push_back(std::make_pair(q, t));
  covariance_blocks.push_back(std::make_pair(t, t));
  if (!covariance.Compute(covariance_blocks, &problem)) { std::printf("covariance not computed\n"); return 1; }
  double cov_qq[4 * 4], cov_qt[4 * 3], cov_tt[3 * 3], tan_qq[3 * 3], tan_qt[3 * 3], full[7 * 7], tan_full[6 * 6];
  bool ok = covariance.GetCovarianceBlock(q, q, cov_qq) && covariance.GetCovarianceBlock(q, t, cov_qt) &&
            covariance.GetCovarianceBlock(t, t, cov_tt) && covariance.GetCovarianceBlockInTangentSpace(q, q, tan_qq) &&
            covariance.GetCovarianceBlockInTangentSpace(q, t, tan_qt);
  ok = ok && covariance.GetCovarianceMatrix({q, t}, full) && covariance.GetCovarianceMatrixInTangentSpace({q, t}, tan_full);
  double unused[16];
  ok = ok && !covariance.GetCovarianceBlock(t, e_disTrans.data(), unused);  // not a computed pair
  if (!ok) { std::printf("covariance blocks missing\n"); return 1; }
  print("q", q, 4);
  print("t", t, 3);
  print("qq", cov_qq, 16);
  print("qt", cov_qt, 12);
  print("tt", cov_tt, 9);
  print("tangent_qq", tan_qq, 9);
  print("tangent_qt", tan_qt, 9);
  print("full", full, 49);
  print("tangent", tan_full, 36);
  return 0;
}
