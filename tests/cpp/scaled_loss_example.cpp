// Per-block weights the way Ceres' documentation writes them: ceres::ScaledLoss around the block's loss (loss_function.h:
// "ScaledLoss: If rho is the wrapped robust loss function, then this simply outputs s -> a * rho(s)"), plain, nested, around
// NULL (a * s) and through a LossFunctionWrapper.  Compiled -std=c++14 -Wall -Werror -fsyntax-only against the facade.
#include <vector>

#include "EAResidue.h"
#include "ceres/ceres.h"

int weighted_problem(const std::vector<double> &a_X, const std::vector<double> &confidence, double *e_disTrans, int rows, int cols,
                     double fx, double fy, double cx, double cy, double *b_quat_a, double *b_t_a) {
  ceres::Grid2D<double, 1> grid(e_disTrans, 0, cols, 0, rows);
  ceres::BiCubicInterpolator<ceres::Grid2D<double, 1>> interpolated_imb_disTrans(grid);
  ceres::Problem problem;
  ceres::LossFunctionWrapper *swappable = new ceres::LossFunctionWrapper(new ceres::CauchyLoss(1.), ceres::TAKE_OWNERSHIP);
  for (size_t i = 0; 4 * i + 3 < a_X.size(); ++i) {
    ceres::CostFunction *cost_function = EAResidue::Create(fx, fy, cx, cy, a_X[4 * i], a_X[4 * i + 1], a_X[4 * i + 2], interpolated_imb_disTrans);
    const double w_i = confidence[i];
    ceres::LossFunction *loss;
    switch (i % 4) {
      case 0: loss = new ceres::ScaledLoss(new ceres::CauchyLoss(1.), w_i, ceres::TAKE_OWNERSHIP); break;
      case 1: loss = new ceres::ScaledLoss(new ceres::ScaledLoss(new ceres::CauchyLoss(1.), 0.5, ceres::TAKE_OWNERSHIP), w_i, ceres::TAKE_OWNERSHIP); break;
      case 2: loss = new ceres::ScaledLoss(NULL, w_i, ceres::TAKE_OWNERSHIP); break;
      default: loss = new ceres::ScaledLoss(swappable, w_i, ceres::DO_NOT_TAKE_OWNERSHIP); break;
    }
    problem.AddResidualBlock(cost_function, loss, b_quat_a, b_t_a);
  }
  problem.SetParameterization(b_quat_a, new ceres::QuaternionParameterization);
  double rho[3];
  ceres::ScaledLoss(NULL, 2.0, ceres::DO_NOT_TAKE_OWNERSHIP).Evaluate(0.5, rho);
  ceres::Solver::Options options;
  ceres::Solver::Summary summary;
  ceres::Solve(options, &problem, &summary);
  double cost = 0.0;
  ceres::Problem::EvaluateOptions eo;
  eo.apply_loss_function = false;  // drops the weights together with the loss
  problem.Evaluate(eo, &cost, NULL, NULL, NULL);
  delete swappable;
  return summary.IsSolutionUsable() && rho[1] == 2.0 ? 0 : 1;
}
