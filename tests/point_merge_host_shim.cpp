// Host shim for tests/test_point_merge_host.py: edge_alignment_amd/csrc/ea_point_merge.h compiled with the host compiler
// (-ffp-contract=off), so the rule the kernels run is checked against tests/point_merge_ref.py without a device.
#include <stdint.h>

#include "ea_point_merge.h"

extern "C" {

// xyz: n x 3 doubles as stored; M: 4 x 4 row-major.  out: n x 3 doubles, each rounded once to float when f32
void point_merge_transform_c(const double *xyz, int64_t n, const double *M, int f32, double *out) {
  for (int64_t i = 0; i < n; ++i) {
    double x, y, z;
    ea::merge_transform(M, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], &x, &y, &z);
    out[3 * i] = f32 ? (double)(float)x : x;
    out[3 * i + 1] = f32 ? (double)(float)y : y;
    out[3 * i + 2] = f32 ? (double)(float)z : z;
  }
}

// the pixel test of step 2 on points already moved and rounded
void point_merge_pixels_c(const double *xyz, int64_t n, double fx, double fy, double cx, double cy, int height, int width, int margin,
                          int *has, int *pu, int *pv) {
  for (int64_t i = 0; i < n; ++i)
    has[i] = ea::merge_pixel(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], fx, fy, cx, cy, height, width, margin, &pu[i], &pv[i]) ? 1 : 0;
}

void point_merge_weights_c(const double *w, int64_t n, double weight_scale, int f32, double *out) {
  for (int64_t i = 0; i < n; ++i) {
    const double v = ea::merge_weight(w[i], weight_scale);
    out[i] = f32 ? (double)(float)v : v;
  }
}

int64_t point_merge_carried_c(int64_t survivors, int64_t max_carried) { return ea::merge_carried(survivors, max_carried); }
int point_merge_weighted_c(int dst_weighted, int src_weighted, double weight_scale) {
  return ea::merge_weighted(dst_weighted != 0, src_weighted != 0, weight_scale) ? 1 : 0;
}
int point_transform_ok_c(const double *M) { return ea::point_transform_error(M) ? 0 : 1; }

int point_merge_ok_c(int require_pixel, int margin, double max_dt, int cell_px, int cell_rule, int height, int width, int64_t max_carried,
                     double weight_scale) {
  ea_point_merge prm;
  prm.require_pixel = require_pixel; prm.margin = margin; prm.max_dt = max_dt; prm.cell_px = cell_px; prm.cell_rule = cell_rule;
  prm.height = height; prm.width = width; prm.max_carried = max_carried; prm.weight_scale = weight_scale;
  return ea::point_merge_ok(&prm) ? 1 : 0;
}

int point_merge_needs_pixel_c(int require_pixel, double max_dt, int cell_px) {
  ea_point_merge prm = {};
  prm.require_pixel = require_pixel; prm.max_dt = max_dt; prm.cell_px = cell_px;
  return ea::point_merge_needs_pixel(&prm) ? 1 : 0;
}

int point_merge_seg_bytes_c(void) { return (int)sizeof(ea::PointMergeSeg); }
int point_transform_seg_bytes_c(void) { return (int)sizeof(ea::PointTransformSeg); }
int point_merge_out_bytes_c(void) { return (int)sizeof(ea::PointMergeOut); }
}
