// Host build of the product's trust-region state machine (ea_lm.h) and covariance code (ea_cov.h) with tangent coordinates
// held constant.  Test-only: the CPU suite compares the shipped masked logic with tests/reduced_lm.py and numpy.
#include <cstring>

#include "ea_cov.h"
#include "ea_lm.h"

extern "C" {

typedef void (*ea_eval_cb)(const double pose[7], double acc[32], void *user);

struct ConstShimOut {
  double x[7];
  int iteration, termination, why, num_successful, num_unsuccessful, num_evals;
  double final_cost, x_norm;
  double it_cost[ea::kTrace];
  double it_radius[ea::kTrace];
  int it_successful[ea::kTrace];
};

// held: bit i = tangent coordinate i of [delta | t] constant; the callback delivers the FULL 6x6 sums (priors included)
int ea_const_host_solve(const ea::LMOptions *o, const double q[4], const double t[3], int held, ea_eval_cb cb, void *user,
                        ConstShimOut *out) {
  ea::LMState s;
  ea::LMCold c;
  ea::LMTrace tr;
  std::memset(&tr, 0, sizeof(tr));
  std::memset(&c, 0, sizeof(c));
  ea::lm_init(&s, o, q, t, 0, held);
  double acc[ea::kAccSlots];
  int guard = o->max_num_iterations + 4;
  while (s.running && guard-- > 0) {
    cb(s.num_evals == 0 ? s.x : s.cand, acc, user);
    ea::lm_feed(&s, &c, &tr, o, acc);
  }
  std::memcpy(out->x, s.x, sizeof(out->x));
  out->iteration = s.iteration; out->termination = s.termination; out->why = s.why;
  out->num_successful = s.num_successful; out->num_unsuccessful = s.num_unsuccessful;
  out->num_evals = s.num_evals; out->final_cost = s.cost; out->x_norm = s.x_norm;
  std::memcpy(out->it_cost, tr.it_cost, sizeof(out->it_cost));
  std::memcpy(out->it_radius, tr.it_radius, sizeof(out->it_radius));
  std::memcpy(out->it_successful, tr.it_successful, sizeof(out->it_successful));
  return s.running ? -1 : 0;
}

void ea_const_host_covariance(const double A[36], double n_invalid, const double q[4], const ea_covariance_options *o, int held,
                              ea_covariance *out) {
  double acc[ea::kAccSlots];
  std::memset(acc, 0, sizeof(acc));
  int k = 0;
  for (int a = 0; a < 6; ++a)
    for (int c = a; c < 6; ++c) acc[ea::kAccJtJ + k++] = A[6 * a + c];
  acc[ea::kAccInvalid] = n_invalid;
  const ea::CovOptions co = {o->algorithm, o->min_reciprocal_condition_number, o->null_space_rank};
  ea::cov_from_acc(acc, q, 1, co, out, held);
}

}  // extern "C"
