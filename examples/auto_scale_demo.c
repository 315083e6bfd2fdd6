/* A loss scale taken from the data (plain C99, include/ea_hip.h alone): the same frame pair with the distance transform as
 * given and multiplied by 255 -- the reference's producers emit both ranges -- first with the reference's fixed
 * CauchyLoss(1.), then with ea_problem_set_loss_auto_scale(2.385, 0.5, 1e-6), i.e. a = 2.385 x median|r| at the start pose.
 *   auto_scale_demo n grid_rows grid_cols fx fy cx cy points.f64 grid.f64
 * (the files of c_abi_demo).  Prints four lines
 *   <fixed|auto> <1|255> q0 q1 q2 q3 t0 t1 t2 iterations a median n_valid
 * (a = the loss scale the solve used, median = the lower median of |r| at the start pose, from ea_problem_residual_quantiles)
 * and a fifth:  ratio_a rotation_gap_fixed translation_gap_fixed rotation_gap_auto translation_gap_auto
 * where a gap is the distance between the x1 and the x255 result (max |dq|, max |dt|).  With the fixed scale the two images
 * are two different problems; with auto scale a follows the image's range and the poses agree. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "ea_hip.h"

static double *read_doubles(const char *path, size_t count) {
  FILE *f = fopen(path, "rb");
  double *buf = (double *)malloc(count * sizeof(double));
  if (!f || !buf || fread(buf, sizeof(double), count, f) != count) {
    fprintf(stderr, "cannot read %lu doubles from %s\n", (unsigned long)count, path);
    exit(2);
  }
  fclose(f);
  return buf;
}

static double gap(const double *a, const double *b, int n) {
  double g = 0.0;
  for (int i = 0; i < n; ++i) g = fmax(g, fabs(a[i] - b[i]));
  return g;
}

int main(int argc, char **argv) {
  if (argc != 10) {
    fprintf(stderr, "usage: %s n grid_rows grid_cols fx fy cx cy points.f64 grid.f64\n", argv[0]);
    return 2;
  }
  const long n = atol(argv[1]);
  const int rows = atoi(argv[2]), cols = atoi(argv[3]);
  ea_camera cam;
  cam.fx = atof(argv[4]); cam.fy = atof(argv[5]); cam.cx = atof(argv[6]); cam.cy = atof(argv[7]);
  double *xyz = read_doubles(argv[8], (size_t)n * 3);
  double *grid = read_doubles(argv[9], (size_t)rows * (size_t)cols);
  double *grid255 = (double *)malloc((size_t)rows * (size_t)cols * sizeof(double));
  if (!grid255) return 2;
  for (size_t i = 0; i < (size_t)rows * (size_t)cols; ++i) grid255[i] = 255.0 * grid[i];

  ea_options opt;
  ea_default_options(&opt);
  double q[2][2][4], t[2][2][3], a_used[2][2];
  for (int mode = 0; mode < 2; ++mode) {        /* 0: CauchyLoss(1.) fixed, 1: auto scale */
    for (int scaled = 0; scaled < 2; ++scaled) {  /* 0: the image as given, 1: x 255 */
      const double q0[4] = {1.0, 0.0, 0.0, 0.0}, t0[3] = {0.0, 0.0, 0.0}, half = 0.5;
      double median = 0.0;
      int64_t n_valid = 0;
      int kind = 0;
      ea_problem *p = NULL;
      ea_summary s;
      double *qq = q[mode][scaled], *tt = t[mode][scaled];
      for (int i = 0; i < 4; ++i) qq[i] = q0[i];
      for (int i = 0; i < 3; ++i) tt[i] = t0[i];
      int rc = ea_problem_create(&p, &cam, EA_F64, 0);
      if (rc == EA_OK) rc = ea_problem_set_points(p, xyz, n, 3);
      if (rc == EA_OK) rc = ea_problem_set_dt(p, scaled ? grid255 : grid, rows, cols);
      if (rc == EA_OK) rc = ea_problem_set_loss(p, EA_LOSS_CAUCHY, 1.0);
      if (rc == EA_OK && mode == 1) rc = ea_problem_set_loss_auto_scale(p, 2.385, 0.5, 1e-6);
      if (rc == EA_OK) rc = ea_problem_residual_quantiles(p, q0, t0, &half, 1, &median, &n_valid);
      if (rc == EA_OK) rc = ea_solve(p, &opt, qq, tt, &s);
      if (rc == EA_OK) rc = ea_problem_get_loss(p, &kind, &a_used[mode][scaled]);
      if (rc != EA_OK) {
        fprintf(stderr, "libea_hip error %d: %s\n", rc, ea_last_error());
        return 1;
      }
      printf("%s %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g %d %.17g %.17g %ld\n", mode ? "auto" : "fixed", scaled ? 255 : 1,
             qq[0], qq[1], qq[2], qq[3], tt[0], tt[1], tt[2], s.num_iterations, a_used[mode][scaled], median, (long)n_valid);
      ea_problem_destroy(p);
    }
  }
  printf("%.17g %.17g %.17g %.17g %.17g\n", a_used[1][1] / a_used[1][0], gap(q[0][0], q[0][1], 4), gap(t[0][0], t[0][1], 3),
         gap(q[1][0], q[1][1], 4), gap(t[1][0], t[1][1], 3));
  free(xyz); free(grid); free(grid255);
  return 0;
}
