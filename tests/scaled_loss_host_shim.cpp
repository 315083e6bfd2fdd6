// Stand-alone host program for tests/test_weights_host.py: ceres::ScaledLoss of the facade (edge_alignment_amd/include/ceres/)
// against Ceres' published definition -- rho -> a rho, a rho', a rho''; NULL = a s; nesting multiplies -- and the grouping of
// residual blocks into families (ceres::ProblemAccess::Families): N blocks with N distinct ScaledLoss factors are ONE family
// whose weights are the factors in block order.  No device and no libea_hip: nothing here builds or solves a problem.
// Built with the host compiler under AddressSanitizer and UBSan, which also watch the ownership rules (a ScaledLoss with
// TAKE_OWNERSHIP deletes what it wraps, ~Problem deletes each loss object once).  Prints "ok <checks>".
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "EAResidue.h"

static int g_checks = 0, g_deleted = 0;
#define CHECK(c)                                                              \
  do {                                                                        \
    ++g_checks;                                                               \
    if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } \
  } while (0)

static bool close(double a, double b) { return std::fabs(a - b) <= 4e-16 * std::fmax(1.0, std::fabs(b)); }

struct CountedCauchy : ceres::CauchyLoss {
  explicit CountedCauchy(double a) : ceres::CauchyLoss(a) {}
  ~CountedCauchy() override { ++g_deleted; }
};

int main() {
  // ---- Evaluate ----
  const double ss[] = {0.0, 1e-9, 0.003, 0.25, 1.0, 7.5, 1e4};
  for (double s : ss) {
    double r[3], in[3];
    {
      ceres::ScaledLoss L(new ceres::CauchyLoss(1.5), 0.37, ceres::TAKE_OWNERSHIP);
      ceres::CauchyLoss(1.5).Evaluate(s, in);
      L.Evaluate(s, r);
      const double b = 2.25, sum = 1.0 + s / b;
      CHECK(r[0] == 0.37 * in[0] && r[1] == 0.37 * in[1] && r[2] == 0.37 * in[2]);
      CHECK(close(r[0], 0.37 * b * std::log(sum)) && close(r[1], 0.37 / sum) && close(r[2], -0.37 / (b * sum * sum)));
      CHECK(r[2] <= 0.0);  // a >= 0 keeps rho'' <= 0: the corrector stays the sqrt(rho') scaling of the kernels
      CHECK(L.ea_kind() == EA_LOSS_CAUCHY && L.ea_scale() == 1.5 && L.ea_weight() == 0.37);
    }
    {
      ceres::HuberLoss H(0.1);
      ceres::ScaledLoss L(&H, 2.0, ceres::DO_NOT_TAKE_OWNERSHIP);
      L.Evaluate(s, r);
      if (s > 0.01) CHECK(close(r[0], 2.0 * (0.2 * std::sqrt(s) - 0.01)) && close(r[1], 2.0 * 0.1 / std::sqrt(s)));
      else CHECK(r[0] == 2.0 * s && r[1] == 2.0 && r[2] == 0.0);
      CHECK(L.ea_kind() == EA_LOSS_HUBER && L.ea_scale() == 0.1 && L.ea_weight() == 2.0);
    }
    {
      ceres::ScaledLoss L(NULL, 0.25, ceres::TAKE_OWNERSHIP);  // NULL = trivial: a s
      L.Evaluate(s, r);
      CHECK(r[0] == 0.25 * s && r[1] == 0.25 && r[2] == 0.0);
      CHECK(L.ea_kind() == EA_LOSS_TRIVIAL && L.ea_weight() == 0.25);
    }
    {
      ceres::ScaledLoss L(new ceres::ScaledLoss(new ceres::CauchyLoss(1.0), 2.0, ceres::TAKE_OWNERSHIP), 3.0, ceres::TAKE_OWNERSHIP);
      L.Evaluate(s, r);
      ceres::CauchyLoss(1.0).Evaluate(s, in);
      CHECK(close(r[0], 6.0 * in[0]) && close(r[1], 6.0 * in[1]) && close(r[2], 6.0 * in[2]));
      CHECK(L.ea_kind() == EA_LOSS_CAUCHY && L.ea_scale() == 1.0 && L.ea_weight() == 6.0);
      ceres::LossFunctionWrapper W(&L, ceres::DO_NOT_TAKE_OWNERSHIP);
      CHECK(W.ea_weight() == 6.0 && W.ea_kind() == EA_LOSS_CAUCHY);
      W.Reset(NULL, ceres::DO_NOT_TAKE_OWNERSHIP);
      CHECK(W.ea_weight() == 1.0 && W.ea_kind() == EA_LOSS_TRIVIAL);
    }
  }
  CHECK(ceres::CauchyLoss(1.0).ea_weight() == 1.0 && ceres::TrivialLoss().ea_weight() == 1.0);

  // ---- families ----
  std::vector<double> texels(16 * 12, 1.0);
  ceres::Grid2D<double, 1> grid(texels.data(), 0, 16, 0, 12);
  ceres::BiCubicInterpolator<ceres::Grid2D<double, 1>> interp(grid);
  double q[4] = {1, 0, 0, 0}, t[3] = {0, 0, 0};
  const int N = 57;
  {
    ceres::Problem problem;
    for (int i = 0; i < N; ++i)
      problem.AddResidualBlock(EAResidue::Create(10, 10, 8, 6, 0.01 * i, -0.02 * i, 1.0 + i, interp),
                               new ceres::ScaledLoss(new CountedCauchy(1.), 0.5 + 0.03125 * i, ceres::TAKE_OWNERSHIP), q, t);
    std::vector<ceres::ProblemAccess::Family> fams;
    std::string err;
    CHECK(ceres::ProblemAccess::Families(&problem, &fams, &err));
    CHECK(fams.size() == 1);  // N distinct weights, ONE family = one GPU problem
    CHECK(fams[0].weighted && (int)fams[0].weights.size() == N && (int)fams[0].idx.size() == N && (int)fams[0].xyz.size() == 3 * N);
    for (int i = 0; i < N; ++i) {
      CHECK(fams[0].weights[(size_t)i] == 0.5 + 0.03125 * i && fams[0].idx[(size_t)i] == i);
      CHECK(fams[0].xyz[3 * (size_t)i + 2] == 1.0 + i);
    }
    CHECK(g_deleted == 0);
  }
  CHECK(g_deleted == N);  // ~Problem deleted every ScaledLoss once, each ScaledLoss what it wrapped
  {
    // weights all 1 (and plain losses): nothing to upload; a different inner loss is another family; a zero weight is allowed
    ceres::Problem problem;
    for (int i = 0; i < 6; ++i)
      problem.AddResidualBlock(EAResidue::Create(10, 10, 8, 6, 0, 0, 1.0 + i, interp),
                               i % 2 ? (ceres::LossFunction *)new ceres::CauchyLoss(1.)
                                     : (ceres::LossFunction *)new ceres::ScaledLoss(new ceres::CauchyLoss(1.), 1.0, ceres::TAKE_OWNERSHIP), q, t);
    problem.AddResidualBlock(EAResidue::Create(10, 10, 8, 6, 0, 0, 9.0, interp), new ceres::ScaledLoss(new ceres::HuberLoss(0.1), 0.0, ceres::TAKE_OWNERSHIP), q, t);
    problem.AddResidualBlock(EAResidue::Create(10, 10, 8, 6, 0, 0, 9.5, interp), new ceres::ScaledLoss(NULL, 4.0, ceres::TAKE_OWNERSHIP), q, t);
    problem.AddResidualBlock(EAResidue::Create(10, 10, 8, 6, 0, 0, 9.7, interp), NULL, q, t);
    std::vector<ceres::ProblemAccess::Family> fams;
    std::string err;
    CHECK(ceres::ProblemAccess::Families(&problem, &fams, &err));
    CHECK(fams.size() == 3);
    CHECK(!fams[0].weighted && fams[0].weights.size() == 6);
    CHECK(fams[1].weighted && fams[1].weights.size() == 1 && fams[1].weights[0] == 0.0);
    CHECK(fams[2].weighted && fams[2].weights.size() == 2 && fams[2].weights[0] == 4.0 && fams[2].weights[1] == 1.0);
  }
  {
    ceres::Problem problem;
    problem.AddResidualBlock(EAResidue::Create(10, 10, 8, 6, 0, 0, 1.0, interp), new ceres::ScaledLoss(new ceres::CauchyLoss(1.), -0.5, ceres::TAKE_OWNERSHIP), q, t);
    std::vector<ceres::ProblemAccess::Family> fams;
    std::string err;
    CHECK(!ceres::ProblemAccess::Families(&problem, &fams, &err));  // a < 0 fails Build with a message
    CHECK(err.find("ScaledLoss") != std::string::npos);
  }
  std::printf("ok %d\n", g_checks);
  return 0;
}
