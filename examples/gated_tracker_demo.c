/* The depth gate inside the multi-stream tracker (plain C99, include/ea_hip.h alone): ea_tracker_batch_set_depth_gate on two
 * streams of a short synthetic sequence, the Canny flavour.  Both streams see a wall of blocks at 1.5 - 2.5 m that moves a pixel
 * to the right per push; from the second push on a box of another colour at 0.6 m stands in front of part of stream 0's wall
 * and moves the other way.  Every solve is preceded by the gate at the pose the stream starts from, against the pushed depth:
 * the reference points that now lie behind the box are OCCLUDED and get weight 0 (the default parameters).
 *   gated_tracker_demo [dump_dir]
 * Prints a first line
 *   frames streams pushes height width fx fy cx cy
 * and one line per push and stream:
 *   push stream aligned q0 q1 q2 q3 t0 t1 t2 n n_behind n_outside n_unknown n_consistent n_occluded n_free
 * With dump_dir the frames it pushed are written there, push-major: bgr.u8 (height x width x 3 bytes each), depth.u16
 * (depth / 5000 = metres). */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ea_hip.h"

#define STREAMS 2
#define PUSHES 4
#define H 48
#define W 64

/* the wall: blocks of 8 x 8 pixels, shade and depth a function of the block, `shift` pixels to the right */
static void wall(uint8_t *bgr, uint16_t *depth, int shift, int stream) {
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const int bx = (x - shift + 64) / 8, by = y / 8;
      const unsigned h = (unsigned)(bx * 37 + by * 101 + stream * 17) * 2654435761u;
      uint8_t *p = bgr + 3 * ((size_t)y * W + x);
      p[0] = (uint8_t)(40 + (h >> 24) % 160); p[1] = (uint8_t)(40 + (h >> 16) % 160); p[2] = (uint8_t)(40 + (h >> 8) % 160);
      depth[(size_t)y * W + x] = (uint16_t)(7500 + 1250 * ((bx + by) % 5));
    }
}

/* the box in front of it */
static void box(uint8_t *bgr, uint16_t *depth, int push) {
  for (int y = 12; y < 34; ++y)
    for (int x = 30 - 2 * push; x < 52 - 2 * push; ++x) {
      uint8_t *p = bgr + 3 * ((size_t)y * W + x);
      p[0] = 230; p[1] = 30; p[2] = 120;
      depth[(size_t)y * W + x] = 3000;
    }
}

static int dump(const char *dir, const char *name, const void *data, size_t bytes) {
  char path[1024];
  if (strlen(dir) + strlen(name) + 2 > sizeof(path)) return 0;
  sprintf(path, "%s/%s", dir, name);
  FILE *f = fopen(path, "wb");
  if (!f) return 0;
  const size_t done = fwrite(data, 1, bytes, f);
  return fclose(f) == 0 && done == bytes;
}

int main(int argc, char **argv) {
  if (argc > 2) {
    fprintf(stderr, "usage: %s [dump_dir]\n", argv[0]);
    return 2;
  }
  static uint8_t bgr[PUSHES][STREAMS][H * W * 3];
  static uint16_t depth[PUSHES][STREAMS][H * W];
  for (int k = 0; k < PUSHES; ++k)
    for (int i = 0; i < STREAMS; ++i) {
      wall(bgr[k][i], depth[k][i], k, i);
      if (i == 0 && k >= 1) box(bgr[k][i], depth[k][i], k);
    }
  if (argc == 2 && !(dump(argv[1], "bgr.u8", bgr, sizeof(bgr)) && dump(argv[1], "depth.u16", depth, sizeof(depth)))) {
    fprintf(stderr, "cannot write the frames to %s\n", argv[1]);
    return 2;
  }
  ea_camera cams[STREAMS];
  for (int i = 0; i < STREAMS; ++i) {
    cams[i].fx = 58.0; cams[i].fy = 58.0; cams[i].cx = 31.5; cams[i].cy = 23.5;
  }
  printf("frames %d %d %d %d %.17g %.17g %.17g %.17g\n", STREAMS, PUSHES, H, W, cams[0].fx, cams[0].fy, cams[0].cx, cams[0].cy);

  ea_tracker_batch *tb = NULL;
  ea_options opt;
  ea_depth_gate_params gate;
  ea_default_options(&opt);
  ea_default_depth_gate_params(&gate); /* radius 1, 2 cm + 2 %, occluded and free points weigh 0 */
  int rc = ea_tracker_batch_create(&tb, cams, STREAMS, EA_F64, 0, /*flavour: Canny*/ 1, 0);
  if (rc == EA_OK) rc = ea_tracker_batch_set_depth_gate(tb, &gate); /* before the first push */
  static ea_summary sums[STREAMS];
  for (int k = 0; rc == EA_OK && k < PUSHES; ++k) {
    const uint8_t *b[STREAMS];
    const void *d[STREAMS];
    double q[STREAMS * 4], t[STREAMS * 3];
    int aligned[STREAMS];
    for (int i = 0; i < STREAMS; ++i) {
      b[i] = bgr[k][i];
      d[i] = depth[k][i];
    }
    rc = ea_tracker_batch_push_frames(tb, b, d, H, W, 5000.0, &opt, q, t, sums, aligned);
    for (int i = 0; rc == EA_OK && i < STREAMS; ++i) {
      ea_depth_gate_stats st;
      rc = ea_tracker_batch_last_depth_gate(tb, 0, i, &st);
      if (rc != EA_OK) break;
      printf("%d %d %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g %ld %ld %ld %ld %ld %ld %ld\n", k + 1, i, aligned[i], q[4 * i],
             q[4 * i + 1], q[4 * i + 2], q[4 * i + 3], t[3 * i], t[3 * i + 1], t[3 * i + 2], (long)st.n, (long)st.n_behind,
             (long)st.n_outside, (long)st.n_unknown, (long)st.n_consistent, (long)st.n_occluded, (long)st.n_free);
    }
  }
  if (rc != EA_OK) {
    fprintf(stderr, "libea_hip error %d: %s\n", rc, ea_last_error());
    return 1;
  }
  ea_tracker_batch_destroy(tb);
  return 0;
}
