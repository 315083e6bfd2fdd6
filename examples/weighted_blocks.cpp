// examples/weighted_blocks.cpp — one weight per residual block, the Ceres way:
//   problem.AddResidualBlock(cost, new ceres::ScaledLoss(new ceres::CauchyLoss(1.), w_i, ceres::TAKE_OWNERSHIP), q, t);
// on the solve block of edge_align_test1 (standalone_test1.cpp has the unweighted text).  N blocks with N different
// weights stay ONE residual family, i.e. one GPU problem whose per-point weights are the ScaledLoss factors
// (ea_problem_set_weights).  Input: the binary file of standalone_test1.cpp.  The weights come from a 64-bit linear
// congruential generator so that a test can restate them:
//   s <- s * 6364136223846793005 + 1442695040888963407 (mod 2^64),  w = 2 * (s >> 40) / 2^24   in [0, 2)
// starting from s = seed, one step per block.
// Output: one line "q0 q1 q2 q3 t0 t1 t2 iterations termination initial_cost final_cost gpu_problems blocks evaluate_cost".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "EAResidue.h"

int main(int argc, char **argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s problem.bin [stride] [seed]\n", argv[0]); return 2; }
  const int stride = argc > 2 ? std::atoi(argv[2]) : 30;
  uint64_t state = argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 1;
  std::FILE *f = std::fopen(argv[1], "rb");
  if (!f) { std::perror("open"); return 2; }
  int32_t N, rows, cols;
  double fx, fy, cx, cy;
  if (std::fread(&N, 4, 1, f) != 1 || std::fread(&rows, 4, 1, f) != 1 || std::fread(&cols, 4, 1, f) != 1) return 2;
  if (std::fread(&fx, 8, 1, f) != 1 || std::fread(&fy, 8, 1, f) != 1 || std::fread(&cx, 8, 1, f) != 1 || std::fread(&cy, 8, 1, f) != 1) return 2;
  std::vector<double> a_X(4 * (size_t)N), e_disTrans((size_t)rows * cols);
  if (std::fread(a_X.data(), 8, a_X.size(), f) != a_X.size()) return 2;
  if (std::fread(e_disTrans.data(), 8, e_disTrans.size(), f) != e_disTrans.size()) return 2;
  std::fclose(f);

  ceres::Grid2D<double, 1> grid(e_disTrans.data(), 0, cols, 0, rows);
  ceres::BiCubicInterpolator<ceres::Grid2D<double, 1>> interpolated_imb_disTrans(grid);
  double b_quat_a[4] = {1, 0, 0, 0}, b_t_a[3] = {0, 0, 0};

  ceres::Problem problem;
  int count = 0;
  for (int i = 0; i < N; i += stride) {
    state = state * 6364136223846793005ULL + 1442695040888963407ULL;
    const double w_i = 2.0 * (double)(state >> 40) / 16777216.0;
    ceres::CostFunction *cost_function =
        EAResidue::Create(fx, fy, cx, cy, a_X[4 * (size_t)i + 0], a_X[4 * (size_t)i + 1], a_X[4 * (size_t)i + 2], interpolated_imb_disTrans);
    problem.AddResidualBlock(cost_function, new ceres::ScaledLoss(new ceres::CauchyLoss(1.), w_i, ceres::TAKE_OWNERSHIP), b_quat_a, b_t_a);
    count++;
  }
  problem.SetParameterization(b_quat_a, new ceres::QuaternionParameterization);

  double cost0 = -1.0;
  const bool eval_ok = problem.Evaluate(ceres::Problem::EvaluateOptions(), &cost0, NULL, NULL, NULL);

  ceres::Solver::Options options;
  ceres::Solver::Summary summary;
  ceres::Solve(options, &problem, &summary);
  std::cerr << summary.FullReport() << "\n";

  std::printf("%.17g %.17g %.17g %.17g %.17g %.17g %.17g %d %d %.17g %.17g %d %d %.17g\n", b_quat_a[0], b_quat_a[1], b_quat_a[2],
              b_quat_a[3], b_t_a[0], b_t_a[1], b_t_a[2], summary.num_successful_steps + summary.num_unsuccessful_steps,
              (int)summary.termination_type, summary.initial_cost, summary.final_cost, summary.ea_num_gpu_problems /* what Solve built */, count,
              eval_ok ? cost0 : -1.0);
  return summary.termination_type == ceres::FAILURE ? 1 : 0;
}
