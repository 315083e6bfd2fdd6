/* N cameras pushed in lock-step (plain C99, include/ea_hip.h alone): ea_tracker_batch on three streams cut from one recorded
 * sequence -- stream 0 plays it forward, stream 1 backward, stream 2 forward from its second frame (wrapping round) -- with the
 * Canny flavour.  Every push hands the tracker one frame per stream; each frame passes the edge detection once and serves
 * first as the current side of its stream's solve, then as the next reference.
 *   multi_tracker_demo height width fx fy cx cy frames bgr.u8 depth.u16
 * bgr.u8: `frames` raw height x width x 3 colour frames back to back, depth.u16: as many height x width uint16 depth frames
 * (depth / 5000 = metres).  Prints one line per push and stream:
 *   push stream aligned q0 q1 q2 q3 t0 t1 t2 iterations final_cost
 * (the pose of the stream's previous frame in its new frame's coordinates; identity while nothing is aligned) and a last line
 *   edge_passes hysteresis_rounds aligned        of the last push: 1 edge-detection chain for all streams, however many solve. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "ea_hip.h"

#define STREAMS 3

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
  ea_camera cams[STREAMS];
  for (int i = 0; i < STREAMS; ++i) {
    cams[i].fx = atof(argv[3]); cams[i].fy = atof(argv[4]); cams[i].cx = atof(argv[5]); cams[i].cy = atof(argv[6]);
  }
  const size_t np = (size_t)H * (size_t)W;
  const uint8_t *bgr = (const uint8_t *)read_file(argv[8], (size_t)frames * np * 3, 0);
  const uint16_t *depth = (const uint16_t *)read_file(argv[9], (size_t)frames * np * 2, 0);

  ea_tracker_batch *tb = NULL;
  ea_options opt;
  ea_default_options(&opt);
  int rc = ea_tracker_batch_create(&tb, cams, STREAMS, EA_F64, 0, /*flavour: Canny*/ 1, 0);
  for (int i = 0; rc == EA_OK && i < STREAMS; ++i) rc = ea_problem_set_loss(ea_tracker_batch_problem(tb, i), EA_LOSS_CAUCHY, 1.0);
  static ea_summary sums[STREAMS]; /* (an ea_summary carries its iteration trace: ~7 KB each) */
  for (int k = 0; rc == EA_OK && k < frames; ++k) {
    const int pick[STREAMS] = {k, frames - 1 - k, (k + 1) % frames};
    const uint8_t *b[STREAMS];
    const void *d[STREAMS];
    double q[STREAMS * 4], t[STREAMS * 3];
    int aligned[STREAMS];
    for (int i = 0; i < STREAMS; ++i) {
      b[i] = bgr + (size_t)pick[i] * np * 3;
      d[i] = depth + (size_t)pick[i] * np;
    }
    rc = ea_tracker_batch_push_frames(tb, b, d, H, W, 5000.0, &opt, q, t, sums, aligned);
    for (int i = 0; rc == EA_OK && i < STREAMS; ++i)
      printf("%d %d %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g %d %.17g\n", k + 1, i, aligned[i], q[4 * i], q[4 * i + 1],
             q[4 * i + 2], q[4 * i + 3], t[3 * i], t[3 * i + 1], t[3 * i + 2], sums[i].num_iterations, sums[i].final_cost);
  }
  int64_t passes = 0, rounds = 0, solved = 0;
  if (rc == EA_OK) rc = ea_tracker_batch_get_info(tb, "edge_passes", &passes);
  if (rc == EA_OK) rc = ea_tracker_batch_get_info(tb, "hysteresis_rounds", &rounds);
  if (rc == EA_OK) rc = ea_tracker_batch_get_info(tb, "aligned", &solved);
  if (rc != EA_OK) {
    fprintf(stderr, "libea_hip error %d: %s\n", rc, ea_last_error());
    return 1;
  }
  printf("%ld %ld %ld\n", (long)passes, (long)rounds, (long)solved);
  ea_tracker_batch_destroy(tb);
  ea_host_free((void *)bgr);
  ea_host_free((void *)depth);
  return 0;
}
