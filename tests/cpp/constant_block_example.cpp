// Problem::SetParameterBlockConstant / SubsetParameterization through the facade on the reference's test1 problem: argv[3]
// selects what is held -- 0 nothing, 1 SetParameterBlockConstant(t), 2 SetParameterBlockConstant(q), 3
// SubsetParameterization(3, {1, 2}) on t, 4 both blocks constant, 5 SubsetParameterization on q (unsupported: the solve must
// say so).  Input: the problem file of examples/standalone_test1.cpp.  Prints the solved pose, the summary's counts, the
// covariance blocks and the report line by line.  Compiled -std=c++14 -Wall -Werror.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "EAResidue.h"
#include "ceres/ceres.h"

static void print(const char *name, const double *v, int n) {
  std::printf("%s", name);
  for (int i = 0; i < n; ++i) std::printf(" %.17g", v[i]);
  std::printf("\n");
}

int main(int argc, char **argv) {
  if (argc < 5) { std::fprintf(stderr, "usage: %s problem.bin stride mode q0w q0x q0y q0z t0x t0y t0z\n", argv[0]); return 2; }
  const int stride = std::atoi(argv[2]), mode = std::atoi(argv[3]);
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
  for (int i = 0; i < 4 && 4 + i < argc; ++i) q[i] = std::atof(argv[4 + i]);
  for (int i = 0; i < 3 && 8 + i < argc; ++i) t[i] = std::atof(argv[8 + i]);
  ceres::Problem problem;
  for (int i = 0; i < N; i += stride)
    problem.AddResidualBlock(EAResidue::Create(fx, fy, cx, cy, a_X[4 * (size_t)i], a_X[4 * (size_t)i + 1], a_X[4 * (size_t)i + 2], interp),
                             new ceres::CauchyLoss(1.), q, t);
  problem.SetParameterization(q, new ceres::QuaternionParameterization);
  std::vector<int> held;
  held.push_back(1);
  held.push_back(2);
  if (mode == 1 || mode == 4) problem.SetParameterBlockConstant(t);
  if (mode == 2 || mode == 4) problem.SetParameterBlockConstant(q);
  if (mode == 3) problem.SetParameterization(t, new ceres::SubsetParameterization(3, held));
  if (mode == 5) {
    std::vector<int> one(1, 0);
    problem.SetParameterization(q, new ceres::SubsetParameterization(4, one));
  }
  const double flags[2] = {problem.IsParameterBlockConstant(q) ? 1.0 : 0.0, problem.IsParameterBlockConstant(t) ? 1.0 : 0.0};
  ceres::Solver::Options options;
  ceres::Solver::Summary summary;
  ceres::Solve(options, &problem, &summary);
  if (summary.termination_type == ceres::FAILURE) { std::printf("failed %s\n", summary.message.c_str()); return mode == 5 ? 0 : 1; }
  const double counts[7] = {(double)summary.num_parameter_blocks, (double)summary.num_parameters, (double)summary.num_effective_parameters,
                            (double)summary.num_parameter_blocks_reduced, (double)summary.num_parameters_reduced,
                            (double)summary.num_effective_parameters_reduced,
                            (double)(summary.num_successful_steps + summary.num_unsuccessful_steps)};
  const double costs[2] = {summary.initial_cost, summary.final_cost};
  print("q", q, 4);
  print("t", t, 3);
  print("constant", flags, 2);
  print("counts", counts, 7);
  print("costs", costs, 2);
  std::printf("reduced_in_report %d\n", std::strstr(summary.FullReport().c_str(), "Reduced") ? 1 : 0);
  // SetParameterBlockVariable gives the block back (no second solve: the flag only)
  problem.SetParameterBlockVariable(t);
  std::printf("t_variable_again %d\n", problem.IsParameterBlockConstant(t) ? 0 : 1);
  if (mode == 1 || mode == 4) problem.SetParameterBlockConstant(t);
  ceres::Covariance::Options copt;
  copt.algorithm_type = ceres::DENSE_SVD;
  ceres::Covariance covariance(copt);
  std::vector<std::pair<const double *, const double *>> blocks;
  blocks.push_back(std::make_pair((const double *)q, (const double *)q));
  blocks.push_back(std::make_pair((const double *)q, (const double *)t));
  blocks.push_back(std::make_pair((const double *)t, (const double *)t));
  if (!covariance.Compute(blocks, &problem)) { std::printf("covariance failed\n"); return 1; }
  double qq[16], qt[12], tt[9];
  covariance.GetCovarianceBlock(q, q, qq);
  covariance.GetCovarianceBlock(q, t, qt);
  covariance.GetCovarianceBlock(t, t, tt);
  print("cov_qq", qq, 16);
  print("cov_qt", qt, 12);
  print("cov_tt", tt, 9);
  return 0;
}
