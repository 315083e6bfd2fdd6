// ea_point_merge.h — carrying reference points between frames (ea_*_transform_points, ea_*_merge_points) as pure logic: the
// argument checks, the transform of a stored point, the margin test on top of ea_point_select.h's pixel, and the arithmetic of
// the stats.  Shared by the kernels (ea_point_transform_kernel, ea_point_merge_*_kernel), the host driver (ea_segments.hip)
// and a host shim without a device (tests/point_merge_host_shim.cpp), which holds it to tests/point_merge_ref.py bit for bit.
//
// include/ea_hip.h states the arithmetic.  Everything here is fp64 in that order with no contracted multiply-add (EA_FP_EXACT,
// ea_reproject.h; the g++ shim is built with -ffp-contract=off).
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/ea_hip.h"
#include "ea_point_select.h"
#include "ea_reproject.h"
#include "ea_types.h"

namespace ea {

constexpr int kPointMergeThreads = kPointSelectThreads;  // lanes of a workgroup of the point passes: one per point

// ---- argument checks (host; NULL = fine, else what is wrong) ---------------------------------------------------------------

// a_T_o / dst_T_src: every entry finite, the last row exactly 0 0 0 1 (reproject_pose_ok's rule)
inline const char *point_transform_error(const double m[16]) {
  if (!reproject_pose_ok(m)) return "the matrix must be finite with a last row of exactly 0 0 0 1";
  return nullptr;
}

inline const char *point_merge_error(const ea_point_merge *prm) {
  if (prm->require_pixel != 0 && prm->require_pixel != 1) return "require_pixel must be 0 or 1";
  if (prm->margin < 0) return "margin must be >= 0";
  if (prm->max_dt != prm->max_dt) return "max_dt must not be NaN (< 0: off)";
  if (prm->cell_px < 0 || prm->cell_px > kPointSelectMaxCellPx) return "cell_px must lie in 0..4096";
  if (prm->cell_rule != EA_CELL_FIRST && prm->cell_rule != EA_CELL_NEAREST) return "cell_rule must be EA_CELL_FIRST or EA_CELL_NEAREST";
  if (prm->height < 0 || prm->width < 0) return "height and width must be >= 0";
  if ((prm->height == 0) != (prm->width == 0)) return "height and width must be given together (0, 0: the DT image's extent)";
  if (prm->cell_px > 0 && prm->height > 0 && point_selection_cells(prm->cell_px, prm->height, prm->width) > kPointSelectMaxCells)
    return "more than 2^26 cells";
  if (prm->max_carried < 0) return "max_carried must be >= 0";
  if (!(prm->weight_scale > 0.0 && prm->weight_scale <= 1.7976931348623157e308)) return "weight_scale must be > 0 and finite";
  return nullptr;
}

inline bool point_merge_ok(const ea_point_merge *prm) { return prm && !point_merge_error(prm); }

// step 2 applies: asked for, or implied by the edge test or the cell step
inline bool point_merge_needs_pixel(const ea_point_merge *prm) {
  return prm->require_pixel != 0 || prm->max_dt >= 0.0 || prm->cell_px > 0;
}

// ---- the transform of a stored point (step B's first line of ea_*_reproject) ---------------------------------------------------

// M: rows 0-2 of the matrix, row-major.  x' = ((M00 x + M01 y) + M02 z) + M03, y' and z' alike
EA_HD EA_SEL_INLINE void merge_transform(const double *M, double x, double y, double z, double *ox, double *oy, double *oz) {
  EA_FP_EXACT
  *ox = ((M[0] * x + M[1] * y) + M[2] * z) + M[3];
  *oy = ((M[4] * x + M[5] * y) + M[6] * z) + M[7];
  *oz = ((M[8] * x + M[9] * y) + M[10] * z) + M[11];
}

// ---- the pixel test of a carried point (step 2) ---------------------------------------------------------------------------------

// select_pixel on the ROUNDED point, and at least `margin` pixels inside the extent
EA_HD EA_SEL_INLINE bool merge_pixel(double x, double y, double z, double fx, double fy, double cx, double cy, int height, int width,
                                     int margin, int *pu, int *pv) {
  if (!select_pixel(x, y, z, fx, fy, cx, cy, height, width, pu, pv)) return false;
  return *pu >= margin && *pu < width - margin && *pv >= margin && *pv < height - margin;
}

// a carried weight: one IEEE multiplication in double (rounded to the dtype on store)
EA_HD EA_SEL_INLINE double merge_weight(double w_src, double weight_scale) {
  EA_FP_EXACT
  return w_src * weight_scale;
}

// ---- the stats ----------------------------------------------------------------------------------------------------------------------

// survivors of steps 1-4 against the cap
EA_HD EA_SEL_INLINE int64_t merge_carried(int64_t survivors, int64_t max_carried) {
  return max_carried > 0 && survivors > max_carried ? max_carried : survivors;
}
// is the merged set weighted?
inline bool merge_weighted(bool dst_weighted, bool src_weighted, double weight_scale) {
  return dst_weighted || src_weighted || weight_scale != 1.0;
}

// ---- what the kernels are handed ------------------------------------------------------------------------------------------------

// ea_point_transform_kernel: one segment per problem of the call
struct PointTransformSeg {
  void *x, *y, *z;  // n each, in the problem dtype, rewritten in place
  int32_t n, pad_;
  double M[12];
};

// ea_point_merge_*_kernel: one segment per dst problem of the call
struct PointMergeSeg {
  const void *x, *y, *z;        // dst's stored points, n_dst each; its weights w_dst elements behind z
  const void *sx, *sy, *sz;     // src's, n_src each; its weights w_src elements behind sz
  void *ox, *oy, *oz;           // room for n_dst + n_src each; the weights land w_out elements behind oz
  int64_t w_dst, w_src, w_out;
  int32_t n_dst, n_src;
  int32_t dst_weighted, src_weighted, out_weighted, pad_;
  double M[12];                 // rows 0-2 of dst_T_src
  double fx, fy, cx, cy;        // dst's camera
  int32_t height, width;        // the extent of the pixel test
  int32_t cells_x, pitch;       // pitch: of dst's DT image in texels (the edge test)
  const void *dt;               // dst's padded DT image in the problem dtype (NULL without an edge test)
  unsigned char *occ;           // per cell: 0 = dst occupies it; all ones before the occupancy pass
  unsigned long long *zmin;     // NEAREST: per free cell the smallest bits of z' among the candidates
  unsigned int *imin;           // per free cell the winning src index
  int32_t *block_counts;        // ceil(n_src / kPointMergeThreads) flagged-point counts, turned into offsets by the scan
};
// behind the records: the counters of a segment the device writes (the survivors come from the scan: PointSelectOut)
struct PointMergeOut { unsigned long long no_pixel, off_edge, occupied, lost_cell; };

}  // namespace ea
