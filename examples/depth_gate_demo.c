/* The depth-consistency gate around one solve, from plain C (C99): an RGB-D frame pair -- the bundled pair of
 * tests/golden/rgbd, say: reference = frame 1, current = frame 2 with its depth -- goes through the Canny producers, the
 * current frame's depth is handed to the problem, and the gate runs at the identity (writing occlusion weights), then the
 * pose is solved with those weights and the gate runs again at the solved pose.
 *   depth_gate_demo height width fx fy cx cy ref_bgr.u8 ref_depth.u16 now_bgr.u8 now_depth.u16
 * The files hold one raw frame each: height x width x 3 colour bytes (B, G, R), height x width uint16 depths (depth / 5000 =
 * metres).  Prints
 *   identity n behind outside unknown consistent occluded free
 *   solved   n behind outside unknown consistent occluded free
 *   pose q0 q1 q2 q3 t0 t1 t2 termination
 * and exits non-zero if the classes of a line do not sum to n. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "ea_hip.h"

static void *read_file(const char *path, size_t bytes) {
  FILE *f = fopen(path, "rb");
  void *buf = malloc(bytes);
  if (!f || !buf || fread(buf, 1, bytes, f) != bytes) {
    fprintf(stderr, "cannot read %lu bytes from %s\n", (unsigned long)bytes, path);
    exit(2);
  }
  fclose(f);
  return buf;
}

static int fail(const char *what, int rc) {
  fprintf(stderr, "%s: libea_hip error %d: %s\n", what, rc, ea_last_error());
  return 1;
}

/* one gate at (q, t), weights written; 0 when the line adds up */
static int gate(ea_problem *p, const char *tag, const double q[4], const double t[3]) {
  double b_T_a[16];
  ea_depth_gate_params prm;
  ea_depth_gate_stats st;
  ea_default_depth_gate_params(&prm); /* radius 1, 2 cm + 2 %, occluded and free points weigh 0, apply */
  int rc = ea_pose_to_matrix(q, t, b_T_a);
  if (rc == EA_OK) rc = ea_problem_depth_gate(p, b_T_a, &prm, NULL, 0, &st);
  if (rc != EA_OK) return fail(tag, rc);
  printf("%s %lld %lld %lld %lld %lld %lld %lld\n", tag, (long long)st.n, (long long)st.n_behind, (long long)st.n_outside,
         (long long)st.n_unknown, (long long)st.n_consistent, (long long)st.n_occluded, (long long)st.n_free);
  return st.n_behind + st.n_outside + st.n_unknown + st.n_consistent + st.n_occluded + st.n_free == st.n ? 0 : 1;
}

int main(int argc, char **argv) {
  if (argc != 11) {
    fprintf(stderr, "usage: %s height width fx fy cx cy ref_bgr.u8 ref_depth.u16 now_bgr.u8 now_depth.u16\n", argv[0]);
    return 2;
  }
  const int H = atoi(argv[1]), W = atoi(argv[2]);
  if (H < 3 || W < 3) return 2;
  ea_camera cam;
  cam.fx = atof(argv[3]); cam.fy = atof(argv[4]); cam.cx = atof(argv[5]); cam.cy = atof(argv[6]);
  const size_t np = (size_t)H * (size_t)W;
  uint8_t *ref_bgr = (uint8_t *)read_file(argv[7], np * 3), *now_bgr = (uint8_t *)read_file(argv[9], np * 3);
  uint16_t *ref_depth = (uint16_t *)read_file(argv[8], np * 2), *now_depth = (uint16_t *)read_file(argv[10], np * 2);

  ea_problem *p = NULL;
  ea_options opt;
  static ea_summary s; /* (an ea_summary carries its iteration trace: ~7 KB) */
  double q[4] = {1.0, 0.0, 0.0, 0.0}, t[3] = {0.0, 0.0, 0.0};
  int rc = ea_problem_create(&p, &cam, EA_F64, 0);
  if (rc == EA_OK) rc = ea_problem_set_ref_frame_canny(p, ref_bgr, ref_depth, H, W, 5000.0, 30.0, 90.0);
  if (rc == EA_OK) rc = ea_problem_set_now_frame_canny(p, now_bgr, NULL, H, W, 30.0, 90.0, 1, 0.0, 1.0);
  if (rc == EA_OK) rc = ea_problem_set_now_depth(p, now_depth, EA_DEPTH_U16, H, W, 5000.0);
  if (rc != EA_OK) return fail("set-up", rc);
  if (gate(p, "identity", q, t) != 0) return 1;
  ea_default_options(&opt);
  rc = ea_solve(p, &opt, q, t, &s); /* with the weights the first gate wrote */
  if (rc != EA_OK) return fail("ea_solve", rc);
  if (gate(p, "solved", q, t) != 0) return 1;
  printf("pose %.17g %.17g %.17g %.17g %.17g %.17g %.17g %d\n", q[0], q[1], q[2], q[3], t[0], t[1], t[2], s.termination);
  ea_problem_destroy(p);
  free(ref_bgr); free(ref_depth); free(now_bgr); free(now_depth);
  return 0;
}
