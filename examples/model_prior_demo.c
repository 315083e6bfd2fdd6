/* Model points, a prior pose and a second-camera term without a read-back, from plain C (C99): the sequence the reference runs
 * before the main solve of its model-alignment tests (standalone_edge_align.cpp:2385-2388),
 *   a_X  = TransformPrior * o_X            ea_problem_transform_points on the first camera's problem
 *   a_X2 = TransformFromFirstCam * a_X     ea_problem_merge_points into the (empty) second-camera problem, every filter off
 * then both residual families on one pose (ea_problem_add_term) and the solve.  Everything is synthetic: the model is the
 * outline of a square, each camera's distance image is the brute-force distance to the outline as that camera sees it at the
 * true pose, and the solve starts at the identity.
 *   model_prior_demo
 * Prints the point counts, the merge's stats and the solve's costs; exits non-zero if a count does not add up or the solve did
 * not lower the cost. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include "ea_hip.h"

#define H 48
#define W 64
#define SIDE 60
#define N (4 * SIDE)

static int fail(const char *what, int rc) {
  fprintf(stderr, "%s: libea_hip error %d: %s\n", what, rc, ea_last_error());
  return 1;
}

static void apply(const double m[16], const double *in, double *out, int n) {
  int i, r;
  for (i = 0; i < n; ++i)
    for (r = 0; r < 3; ++r)
      out[3 * i + r] = ((m[4 * r] * in[3 * i] + m[4 * r + 1] * in[3 * i + 1]) + m[4 * r + 2] * in[3 * i + 2]) + m[4 * r + 3];
}

/* the distance image of a camera: per pixel the distance to the nearest projected point, as ea_problem_set_dt takes it
 * (value(r, c) at data[r * H + c] with r = u, c = v) */
static void distance_image(const ea_camera *cam, const double *xyz, int n, double *data) {
  int u, v, i;
  for (u = 0; u < W; ++u)
    for (v = 0; v < H; ++v) {
      double best = 1e30;
      for (i = 0; i < n; ++i) {
        const double pu = cam->fx * xyz[3 * i] / xyz[3 * i + 2] + cam->cx, pv = cam->fy * xyz[3 * i + 1] / xyz[3 * i + 2] + cam->cy;
        const double d = sqrt((pu - u) * (pu - u) + (pv - v) * (pv - v));
        if (d < best) best = d;
      }
      data[u * H + v] = best;
    }
}

int main(void) {
  /* the model in its own frame: the outline of a square of 0.4 m */
  static double o_X[3 * N], a_X_true[3 * N], a_X2_true[3 * N], moved[3 * N], dt[W * H];
  /* the prior places the model in front of the first camera; the second camera sits 5 cm to the side */
  const double prior[16] = {0.98, -0.199, 0, 0.02, 0.199, 0.98, 0, -0.01, 0, 0, 1, 1.5, 0, 0, 0, 1};
  const double T12[16] = {1, 0, 0, -0.05, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const double T12inv[16] = {1, 0, 0, 0.05, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  /* what the solve should find: a small motion of the model in the first camera's frame */
  const double q_true[4] = {0.9998, 0.0, 0.0, 0.02}, t_true[3] = {0.01, -0.008, 0.0};
  double b_T_a[16], q[4] = {1, 0, 0, 0}, t[3] = {0, 0, 0};
  ea_camera cam;
  ea_problem *p1 = NULL, *p2 = NULL;
  ea_point_merge prm;
  ea_point_merge_stats st;
  ea_options opt;
  ea_summary sum;
  int i, rc;

  cam.fx = 60.0; cam.fy = 60.0; cam.cx = 31.5; cam.cy = 23.5;
  for (i = 0; i < SIDE; ++i) {
    const double s = -0.2 + 0.4 * i / SIDE;
    const double side[4][2] = {{s, -0.2}, {0.2, s}, {-s, 0.2}, {-0.2, -s}};
    int k;
    for (k = 0; k < 4; ++k) {
      o_X[3 * (4 * i + k)] = side[k][0]; o_X[3 * (4 * i + k) + 1] = side[k][1]; o_X[3 * (4 * i + k) + 2] = 0.0;
    }
  }

  /* the images: what each camera sees of the model at the true pose */
  if ((rc = ea_pose_to_matrix(q_true, t_true, b_T_a)) != EA_OK) return fail("ea_pose_to_matrix", rc);
  apply(prior, o_X, moved, N);
  apply(b_T_a, moved, a_X_true, N);
  apply(T12, a_X_true, a_X2_true, N);

  rc = ea_problem_create(&p1, &cam, EA_F64, 0);
  if (rc == EA_OK) rc = ea_problem_create(&p2, &cam, EA_F64, 0);
  if (rc == EA_OK) rc = ea_problem_set_second_camera(p2, T12, T12inv);
  if (rc != EA_OK) return fail("set-up", rc);
  distance_image(&cam, a_X_true, N, dt);
  if ((rc = ea_problem_set_dt(p1, dt, W, H)) != EA_OK) return fail("ea_problem_set_dt", rc);
  distance_image(&cam, a_X2_true, N, dt);
  if ((rc = ea_problem_set_dt(p2, dt, W, H)) != EA_OK) return fail("ea_problem_set_dt", rc);

  /* a_X = TransformPrior * o_X, where the points are */
  if ((rc = ea_problem_set_points(p1, o_X, N, 3)) != EA_OK) return fail("ea_problem_set_points", rc);
  if ((rc = ea_problem_transform_points(p1, prior)) != EA_OK) return fail("ea_problem_transform_points", rc);
  /* a_X2 = TransformFromFirstCam * a_X: a dst without points and every filter off */
  ea_default_point_merge(&prm);
  if ((rc = ea_problem_merge_points(p2, p1, T12, &prm, &st)) != EA_OK) return fail("ea_problem_merge_points", rc);
  printf("points %lld %lld\n", (long long)ea_problem_num_points(p1), (long long)ea_problem_num_points(p2));
  printf("merge %lld %lld %lld %lld\n", (long long)st.n_dst, (long long)st.n_src, (long long)st.carried, (long long)st.n_after);
  if (st.n_dst != 0 || st.n_src != N || st.carried != N || st.n_after != N || ea_problem_num_points(p2) != N) return 1;

  /* both cameras' residual blocks on one pose, and the solve */
  if ((rc = ea_problem_add_term(p1, p2)) != EA_OK) return fail("ea_problem_add_term", rc);
  ea_default_options(&opt);
  if ((rc = ea_solve(p1, &opt, q, t, &sum)) != EA_OK) return fail("ea_solve", rc);
  printf("cost %.6g -> %.6g in %d iterations\n", sum.initial_cost, sum.final_cost, sum.num_iterations);
  printf("q %.5f %.5f %.5f %.5f  t %.5f %.5f %.5f\n", q[0], q[1], q[2], q[3], t[0], t[1], t[2]);
  if (!(sum.final_cost < sum.initial_cost)) return 1;
  ea_problem_destroy(p1);
  ea_problem_destroy(p2);
  return 0;
}
