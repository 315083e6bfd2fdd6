/* Coarse-to-fine tracking of N cameras in lock-step (plain C99, include/ea_hip.h alone): ea_tracker_batch_create_pyramid on two
 * streams cut from one recorded sequence -- stream 0 plays it forward, stream 1 backward -- with three pyramid levels of the
 * ROS chain.  Every push hands the tracker one full-size frame per stream; the frames go up once, one halving chain gives
 * every level its frame, and each aligned stream is solved on its coarsest usable level first, the pose carried down.
 *   pyramid_tracker_demo height width fx fy cx cy halvings frames bgr.u8 depth.f32
 * fx fy cx cy: the camera at the full extent; level l works at (height, width) >> (halvings + l) with the camera scaled by
 * 2^-(halvings + l).  bgr.u8: `frames` raw height x width x 3 colour frames back to back, depth.f32: as many height x width
 * float32 depth frames in metres.  Prints one line per push and stream:
 *   push stream aligned q0 q1 q2 q3 t0 t1 t2 iterations_level0 iterations_level1 iterations_level2 final_cost_level0
 * (-1 iterations: the level was not solved) and a last line
 *   levels edge_passes aligned        of the last push: one edge-detection chain per level for all streams. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "ea_hip.h"

#define STREAMS 2
#define LEVELS 3

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
  if (argc != 11) {
    fprintf(stderr, "usage: %s height width fx fy cx cy halvings frames bgr.u8 depth.f32\n", argv[0]);
    return 2;
  }
  const int H = atoi(argv[1]), W = atoi(argv[2]), halvings = atoi(argv[7]), frames = atoi(argv[8]);
  if (H < 3 || W < 3 || frames < 2 || halvings < 0) return 2;
  ea_camera cams[LEVELS * STREAMS]; /* level-major */
  for (int l = 0; l < LEVELS; ++l)
    for (int i = 0; i < STREAMS; ++i) {
      const double s = 1.0 / (double)(1 << (halvings + l));
      ea_camera *c = &cams[l * STREAMS + i];
      c->fx = atof(argv[3]) * s; c->fy = atof(argv[4]) * s; c->cx = atof(argv[5]) * s; c->cy = atof(argv[6]) * s;
    }
  const size_t np = (size_t)H * (size_t)W;
  const uint8_t *bgr = (const uint8_t *)read_file(argv[9], (size_t)frames * np * 3, 0);
  const float *depth = (const float *)read_file(argv[10], (size_t)frames * np * 4, 0);

  ea_tracker_batch *tb = NULL;
  ea_options opt;
  ea_default_options(&opt);
  int rc = ea_tracker_batch_create_pyramid(&tb, cams, STREAMS, LEVELS, EA_F64, 0, halvings);
  for (int l = 0; rc == EA_OK && l < LEVELS; ++l)
    for (int i = 0; rc == EA_OK && i < STREAMS; ++i)
      rc = ea_problem_set_loss(ea_tracker_batch_level_problem(tb, l, i), EA_LOSS_CAUCHY, 1.0);
  static ea_summary sums[STREAMS], per_level[LEVELS]; /* (an ea_summary carries its iteration trace: ~7 KB each) */
  for (int k = 0; rc == EA_OK && k < frames; ++k) {
    const int pick[STREAMS] = {k, frames - 1 - k};
    const uint8_t *b[STREAMS];
    const void *d[STREAMS];
    double q[STREAMS * 4], t[STREAMS * 3];
    int aligned[STREAMS];
    for (int i = 0; i < STREAMS; ++i) {
      b[i] = bgr + (size_t)pick[i] * np * 3;
      d[i] = depth + (size_t)pick[i] * np;
    }
    rc = ea_tracker_batch_push_frames(tb, b, d, H, W, 0.0, &opt, q, t, sums, aligned);
    for (int i = 0; rc == EA_OK && i < STREAMS; ++i) {
      rc = ea_tracker_batch_last_summaries(tb, i, per_level);
      if (rc != EA_OK) break;
      int its[LEVELS];
      for (int l = 0; l < LEVELS; ++l) /* a level that was not solved has a zeroed summary: no evaluation at all */
        its[l] = per_level[l].num_point_evals == 0 && per_level[l].num_iterations == 0 ? -1 : per_level[l].num_iterations;
      printf("%d %d %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g %d %d %d %.17g\n", k + 1, i, aligned[i], q[4 * i], q[4 * i + 1],
             q[4 * i + 2], q[4 * i + 3], t[3 * i], t[3 * i + 1], t[3 * i + 2], its[0], its[1], its[2], per_level[0].final_cost);
    }
  }
  int64_t levels = 0, passes = 0, solved = 0;
  if (rc == EA_OK) rc = ea_tracker_batch_get_info(tb, "levels", &levels);
  if (rc == EA_OK) rc = ea_tracker_batch_get_info(tb, "edge_passes", &passes);
  if (rc == EA_OK) rc = ea_tracker_batch_get_info(tb, "aligned", &solved);
  if (rc != EA_OK) {
    fprintf(stderr, "libea_hip error %d: %s\n", rc, ea_last_error());
    return 1;
  }
  printf("%ld %ld %ld\n", (long)levels, (long)passes, (long)solved);
  ea_tracker_batch_destroy(tb);
  ea_host_free((void *)bgr);
  ea_host_free((void *)depth);
  return 0;
}
