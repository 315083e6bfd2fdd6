/* Point selection on the device, from plain C (C99): a reference frame -- frame 1 of tests/golden/rgbd, say -- goes through
 * the Laplacian producer (get_aX), and its edge points are thinned where they are, as the reference's tests thin theirs before
 * they build the problem: edge_align_test1's `i += 30`, then one point per cell of cell_px pixels with the stereo tests'
 * iterStep rule on top.
 *   point_selection_demo height width fx fy cx cy ref_bgr.u8 ref_depth.u16 [cell_px [target]]
 * The files hold one raw frame each: height x width x 3 colour bytes (B, G, R), height x width uint16 depths (depth / 5000 =
 * metres).  Prints
 *   stride n_before n_after
 *   cells  n_before no_pixel after_cells n_after stride_used        (with cell_px)
 * -- for the bundled frame `stride 44457 1482`, the reference log's 1482 residual blocks -- and exits non-zero if a line does
 * not add up. */
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

int main(int argc, char **argv) {
  if (argc < 9 || argc > 11) {
    fprintf(stderr, "usage: %s height width fx fy cx cy ref_bgr.u8 ref_depth.u16 [cell_px [target]]\n", argv[0]);
    return 2;
  }
  const int H = atoi(argv[1]), W = atoi(argv[2]);
  if (H < 3 || W < 3) return 2;
  ea_camera cam;
  cam.fx = atof(argv[3]); cam.fy = atof(argv[4]); cam.cx = atof(argv[5]); cam.cy = atof(argv[6]);
  const size_t np = (size_t)H * (size_t)W;
  uint8_t *bgr = (uint8_t *)read_file(argv[7], np * 3);
  uint16_t *depth = (uint16_t *)read_file(argv[8], np * 2);

  ea_problem *p = NULL;
  ea_point_selection prm;
  ea_point_selection_stats st;
  int rc = ea_problem_create(&p, &cam, EA_F64, 0);
  if (rc == EA_OK) rc = ea_problem_set_ref_frame(p, bgr, depth, H, W, 5000.0, 35);
  if (rc != EA_OK) return fail("set-up", rc);
  ea_default_point_selection(&prm);
  prm.stride = 30; /* standalone_edge_align.cpp:267 */
  if ((rc = ea_problem_select_points(p, &prm, &st)) != EA_OK) return fail("ea_problem_select_points", rc);
  printf("stride %lld %lld\n", (long long)st.n_before, (long long)st.n_after);
  if (st.n_after != (st.n_before + 29) / 30 || ea_problem_num_points(p) != st.n_after) return 1;
  if (argc > 9) {
    /* the same frame again: one point per cell, the nearest; the reference frame has no DT image, so the grid is named */
    if ((rc = ea_problem_set_ref_frame(p, bgr, depth, H, W, 5000.0, 35)) != EA_OK) return fail("set-up", rc);
    ea_default_point_selection(&prm);
    prm.cell_px = atoi(argv[9]);
    prm.cell_rule = EA_CELL_NEAREST;
    prm.height = H; prm.width = W;
    prm.target = argc > 10 ? atoll(argv[10]) : 0;
    if ((rc = ea_problem_select_points(p, &prm, &st)) != EA_OK) return fail("ea_problem_select_points", rc);
    printf("cells %lld %lld %lld %lld %lld\n", (long long)st.n_before, (long long)st.no_pixel, (long long)st.after_cells,
           (long long)st.n_after, (long long)st.stride_used);
    if (st.n_after != (st.after_cells + st.stride_used - 1) / st.stride_used || ea_problem_num_points(p) != st.n_after) return 1;
  }
  ea_problem_destroy(p);
  free(bgr); free(depth);
  return 0;
}
