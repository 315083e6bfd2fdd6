/* Keyframe tracking against frame-to-frame tracking (plain C99, include/ea_hip.h alone): one stream of a recorded sequence
 * -- the five bundled RGB-D grabs of tests/golden/rgbd, say -- pushed through ea_tracker_batch twice, Canny flavour: first
 * frame to frame (every pushed frame becomes the reference), then in keyframe mode (the reference is held while enough of it
 * is still seen: ea_tracker_batch_set_keyframes).
 *   keyframe_tracker_demo height width fx fy cx cy frames bgr.u8 depth.u16
 * bgr.u8: `frames` raw height x width x 3 colour frames back to back, depth.u16: as many height x width uint16 depth frames
 * (depth / 5000 = metres).  Prints one line per mode and push:
 *   mode push aligned n n_invalid n_visible n_inlier n_flow mean_flow reason keyframe_push age q0 q1 q2 q3 t0 t1 t2
 * mode 0 = frame to frame, which keeps no statistics (zeros; every push replaces the reference), mode 1 = keyframes; the pose
 * is the one solved in that push against the reference (keyframe) in use during it. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "ea_hip.h"

static void *read_file(const char *path, size_t bytes, int device) {
  FILE *f = fopen(path, "rb");
  void *buf = ea_host_alloc(bytes, device); /* page-locked: the frames go up as direct DMA */
  if (!f || !buf || fread(buf, 1, bytes, f) != bytes) {
    fprintf(stderr, "cannot read %lu bytes from %s\n", (unsigned long)bytes, path);
    exit(2);
  }
  fclose(f);
  return buf;
}

int main(int argc, char **argv) {
  if (argc != 10) {
    fprintf(stderr, "usage: %s height width fx fy cx cy frames bgr.u8 depth.u16\n", argv[0]);
    return 2;
  }
  const int H = atoi(argv[1]), W = atoi(argv[2]), frames = atoi(argv[7]);
  if (H < 3 || W < 3 || frames < 2) return 2;
  ea_camera cam;
  cam.fx = atof(argv[3]); cam.fy = atof(argv[4]); cam.cx = atof(argv[5]); cam.cy = atof(argv[6]);
  const size_t np = (size_t)H * (size_t)W;
  const uint8_t *bgr = (const uint8_t *)read_file(argv[8], (size_t)frames * np * 3, 0);
  const uint16_t *depth = (const uint16_t *)read_file(argv[9], (size_t)frames * np * 2, 0);

  ea_keyframe_params prm;
  ea_default_keyframe_params(&prm); /* min_visible_fraction 0.75, the other rules off */
  prm.min_inlier_fraction = 0.5;
  prm.inlier_residual = 0.05;       /* of a transform normalised to [0, 1] */
  prm.max_frames = 3;
  prm.margin = 2;
  ea_options opt;
  ea_default_options(&opt);
  static ea_summary sum; /* (an ea_summary carries its iteration trace: ~7 KB) */
  int rc = EA_OK;
  for (int mode = 0; rc == EA_OK && mode < 2; ++mode) {
    ea_tracker_batch *tb = NULL;
    rc = ea_tracker_batch_create(&tb, &cam, 1, EA_F64, 0, /*flavour: Canny*/ 1, 0);
    if (rc == EA_OK) rc = ea_problem_set_loss(ea_tracker_batch_problem(tb, 0), EA_LOSS_CAUCHY, 1.0);
    if (rc == EA_OK && mode == 1) rc = ea_tracker_batch_set_keyframes(tb, &prm);
    for (int k = 0; rc == EA_OK && k < frames; ++k) {
      const uint8_t *b = bgr + (size_t)k * np * 3;
      const void *d = depth + (size_t)k * np;
      double q[4], t[3];
      int aligned = 0;
      ea_keyframe_state st = {0, 0, 0, {0, 0, 0, 0, 0, 0.0}};
      rc = ea_tracker_batch_push_frames(tb, &b, &d, H, W, 5000.0, &opt, q, t, &sum, &aligned);
      if (rc == EA_OK && mode == 1) rc = ea_tracker_batch_keyframe_state(tb, 0, &st);
      if (rc != EA_OK) break;
      printf("%d %d %d %ld %ld %ld %ld %ld %.6f %d %ld %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", mode, k + 1, aligned,
             (long)st.stats.n, (long)st.stats.n_invalid, (long)st.stats.n_visible, (long)st.stats.n_inlier, (long)st.stats.n_flow,
             st.stats.n_flow > 0 ? st.stats.sum_flow / (double)st.stats.n_flow : 0.0, st.replaced, (long)st.keyframe_push, st.age,
             q[0], q[1], q[2], q[3], t[0], t[1], t[2]);
    }
    ea_tracker_batch_destroy(tb);
  }
  if (rc != EA_OK) {
    fprintf(stderr, "libea_hip error %d: %s\n", rc, ea_last_error());
    return 1;
  }
  ea_host_free((void *)bgr);
  ea_host_free((void *)depth);
  return 0;
}
