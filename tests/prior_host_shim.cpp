// Host build of the product's NormalPrior code (edge_alignment_amd/csrc/ea_prior.h, the code the LM kernels and the host
// drivers run) and of the facade's QuaternionParameterization::Plus.  Test-only: the CPU suite checks the prior's JtJ, Jtr
// and cost against numpy and its gradient against finite differences without a GPU.
#include <cstring>

#include "ea_prior.h"
#include "ceres/ceres.h"

extern "C" {

// H_q (4x4), b_q (4), H_t (3x3), b_t (3), has_q / has_t, x = (q, t) -> the 32 accumulator slots (zero before the call)
void ea_prior_host_add(const double Hq[16], const double bq[4], int has_q, const double Ht[9], const double bt[3], int has_t,
                       const double x[7], double acc[32]) {
  ea::PriorDesc pr;
  std::memset(&pr, 0, sizeof(pr));
  std::memcpy(pr.Hq, Hq, sizeof(pr.Hq));
  std::memcpy(pr.bq, bq, sizeof(pr.bq));
  std::memcpy(pr.Ht, Ht, sizeof(pr.Ht));
  std::memcpy(pr.bt, bt, sizeof(pr.bt));
  pr.has_q = has_q;
  pr.has_t = has_t;
  ea::prior_add(pr, x, acc);
}

void ea_prior_host_quat_plus(const double x[4], const double delta[3], double out[4]) {
  ceres::QuaternionParameterization().Plus(x, delta, out);
}

}  // extern "C"
