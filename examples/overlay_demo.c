/* The reference's before / after self-check from plain C (C99): reproject + s_overlay "initial.png" / "final.png" and the
 * integer-pixel cost report, around one solve, all on the device.
 *   overlay_demo problem.bin initial.ppm final.ppm
 * problem.bin: the file examples/standalone_test1.cpp reads -- int32 N, rows (image height), cols (image width); double
 * fx, fy, cx, cy; the 4 x N column-major a_X; the rows x cols column-major distance transform (= the Grid2D view).
 * The overlays are painted in upstream's red onto a mid-grey image and written as binary PPM (P6).  Prints two lines,
 *   initial inside outside n | count outside total_cost
 *   final   inside outside n | count outside total_cost
 * the ea_overlay_stats next to ea_problem_pixel_cost's report at the same pose, then the solved pose on a third. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ea_hip.h"

static int fail(const char *what, int rc) {
  fprintf(stderr, "%s: libea_hip error %d: %s\n", what, rc, ea_last_error());
  return 1;
}

/* BGR bytes -> binary PPM (RGB) */
static int write_ppm(const char *path, const uint8_t *bgr, int height, int width) {
  FILE *f = fopen(path, "wb");
  if (!f) return -1;
  fprintf(f, "P6\n%d %d\n255\n", width, height);
  for (size_t i = 0; i < (size_t)height * (size_t)width; ++i) {
    const uint8_t rgb[3] = {bgr[3 * i + 2], bgr[3 * i + 1], bgr[3 * i]};
    if (fwrite(rgb, 1, 3, f) != 3) { fclose(f); return -1; }
  }
  return fclose(f);
}

/* one overlay + one pixel-cost report at (q, t) */
static int report(ea_problem *p, const char *tag, const double q[4], const double t[3], const uint8_t *grey, uint8_t *out,
                  int height, int width, const char *path) {
  double b_T_a[16];
  ea_overlay_stats st;
  ea_pixel_cost pc;
  int rc = ea_pose_to_matrix(q, t, b_T_a);
  if (rc == EA_OK) rc = ea_problem_overlay(p, b_T_a, grey, height, width, NULL, out, &st);
  if (rc == EA_OK) rc = ea_problem_pixel_cost(p, q, t, &pc);
  if (rc != EA_OK) return fail(tag, rc);
  if (write_ppm(path, out, height, width) != 0) { fprintf(stderr, "cannot write %s\n", path); return 1; }
  printf("%s %lld %lld %lld | %lld %lld %.17g\n", tag, (long long)st.inside, (long long)st.outside, (long long)st.n,
         (long long)pc.count, (long long)pc.outside, pc.total_cost);
  return 0;
}

int main(int argc, char **argv) {
  if (argc != 4) {
    fprintf(stderr, "usage: %s problem.bin initial.ppm final.ppm\n", argv[0]);
    return 2;
  }
  FILE *f = fopen(argv[1], "rb");
  int32_t n = 0, rows = 0, cols = 0;
  ea_camera cam;
  if (!f || fread(&n, 4, 1, f) != 1 || fread(&rows, 4, 1, f) != 1 || fread(&cols, 4, 1, f) != 1 ||
      fread(&cam, sizeof(double), 4, f) != 4 || n < 1 || rows < 1 || cols < 1) {
    fprintf(stderr, "cannot read the header of %s\n", argv[1]);
    return 2;
  }
  double *a_X = (double *)malloc((size_t)n * 4 * sizeof(double));
  double *dt = (double *)malloc((size_t)rows * (size_t)cols * sizeof(double));
  const size_t image_bytes = (size_t)rows * (size_t)cols * 3;
  uint8_t *grey = (uint8_t *)malloc(image_bytes), *out = (uint8_t *)malloc(image_bytes);
  if (!a_X || !dt || !grey || !out || fread(a_X, sizeof(double), (size_t)n * 4, f) != (size_t)n * 4 ||
      fread(dt, sizeof(double), (size_t)rows * (size_t)cols, f) != (size_t)rows * (size_t)cols) {
    fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  fclose(f);
  memset(grey, 128, image_bytes);

  ea_problem *p = NULL;
  ea_options opt;
  ea_summary s;
  double q[4] = {1.0, 0.0, 0.0, 0.0}, t[3] = {0.0, 0.0, 0.0};
  int rc = ea_problem_create(&p, &cam, EA_F64, 0);
  if (rc == EA_OK) rc = ea_problem_set_points(p, a_X, n, 4);
  if (rc == EA_OK) rc = ea_problem_set_dt(p, dt, cols, rows);   /* Grid2D rows = the u extent = the image width */
  if (rc != EA_OK) return fail("set-up", rc);
  if (report(p, "initial", q, t, grey, out, rows, cols, argv[2]) != 0) return 1;
  ea_default_options(&opt);
  rc = ea_solve(p, &opt, q, t, &s);
  if (rc != EA_OK) return fail("ea_solve", rc);
  if (report(p, "final", q, t, grey, out, rows, cols, argv[3]) != 0) return 1;
  printf("pose %.17g %.17g %.17g %.17g %.17g %.17g %.17g %d\n", q[0], q[1], q[2], q[3], t[0], t[1], t[2], s.termination);
  ea_problem_destroy(p);
  free(a_X); free(dt); free(grey); free(out);
  return 0;
}
