// ea_point_select.h — device point selection (ea_*_select_points) as pure logic: the argument checks, the pixel of a stored
// point, its cell, and the stride the survivors of the cell step are thinned with.  Shared by the kernels
// (ea_point_select_*_kernel), the host driver (ea_segments.hip) and a host shim without a device
// (tests/point_select_host_shim.cpp), which holds it to tests/point_select_ref.py bit for bit.
//
// include/ea_hip.h states the arithmetic.  Everything here is fp64 in that order with no contracted multiply-add (EA_FP_EXACT,
// ea_reproject.h; the g++ shim is built with -ffp-contract=off) and IEEE divisions.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/ea_hip.h"
#include "ea_reproject.h"
#include "ea_types.h"

#if defined(__HIPCC__)
#define EA_SEL_INLINE __forceinline__
#else
#define EA_SEL_INLINE inline
#endif

namespace ea {

constexpr int kPointSelectThreads = 256;   // lanes of a workgroup of the point passes: one per point
constexpr int kPointSelectScan = 1024;     // lanes of the scan's one workgroup per segment; it walks chunks of this many counts
constexpr int kPointSelectMaxCellPx = 4096;
constexpr int64_t kPointSelectMaxCells = (int64_t)1 << 26;

// ---- argument checks (host; NULL = fine, else what is wrong) ---------------------------------------------------------------

// cells of an extent: ceil(W / c) columns times ceil(H / c) rows
inline int64_t point_selection_cells(int cell_px, int height, int width) {
  const int64_t c = cell_px;
  return ((width + c - 1) / c) * ((height + c - 1) / c);
}

inline const char *point_selection_error(const ea_point_selection *prm) {
  if (prm->cell_px < 0 || prm->cell_px > kPointSelectMaxCellPx) return "cell_px must lie in 0..4096";
  if (prm->cell_rule != EA_CELL_FIRST && prm->cell_rule != EA_CELL_NEAREST) return "cell_rule must be EA_CELL_FIRST or EA_CELL_NEAREST";
  if (prm->outside != 0 && prm->outside != 1) return "outside must be 0 (dropped) or 1 (kept)";
  if (prm->stride < 1) return "stride must be >= 1";
  if (prm->target < 0) return "target must be >= 0";
  if (prm->stride > 1 && prm->target > 0) return "target needs stride == 1";
  if (prm->height < 0 || prm->width < 0) return "height and width must be >= 0";
  if ((prm->height == 0) != (prm->width == 0)) return "height and width must be given together (0, 0: the DT image's extent)";
  if (prm->cell_px > 0 && prm->height > 0 && point_selection_cells(prm->cell_px, prm->height, prm->width) > kPointSelectMaxCells)
    return "more than 2^26 cells";
  return nullptr;
}

inline bool point_selection_ok(const ea_point_selection *prm) { return prm && !point_selection_error(prm); }

// cell_px == 0, stride == 1, target == 0: every point survives in its place
inline bool point_selection_is_identity(const ea_point_selection *prm) {
  return prm->cell_px == 0 && prm->stride == 1 && prm->target == 0;
}

// ---- the pixel of a stored point ---------------------------------------------------------------------------------------------

// The plain pinhole of the problem's own camera at the identity pose, from the point as stored (widened to double): a = x / z,
// b = y / z; u = fx * a, rounded, + cx; v likewise; pu = floor(u + 0.5), pv = floor(v + 0.5).  true: the point has a pixel --
// z > 0 (false for NaN), u and v finite, 0 <= pu < width, 0 <= pv < height, compared in double before any conversion.
EA_HD EA_SEL_INLINE bool select_pixel(double x, double y, double z, double fx, double fy, double cx, double cy, int height, int width,
                                      int *pu_out, int *pv_out) {
  EA_FP_EXACT
  const double a = x / z, b = y / z;
  const double fa = fx * a, fb = fy * b;
  const double u = fa + cx, v = fb + cy;
  const double pu = floor(u + 0.5), pv = floor(v + 0.5);
  const double big = 1.7976931348623157e308;
  const bool finite = u >= -big && u <= big && v >= -big && v <= big;  // (false for NaN)
  const bool has = z > 0.0 && finite && pu >= 0.0 && pu < (double)width && pv >= 0.0 && pv < (double)height;
  *pu_out = has ? (int)pu : -1;
  *pv_out = has ? (int)pv : -1;
  return has;
}

// cells_x = ceil(width / cell_px)
EA_HD EA_SEL_INLINE int select_cells_x(int cell_px, int width) { return (width - 1) / cell_px + 1; }  // (width >= 1)
EA_HD EA_SEL_INLINE int select_cell(int pu, int pv, int cell_px, int cells_x) { return (pv / cell_px) * cells_x + pu / cell_px; }

// ---- the stride step -----------------------------------------------------------------------------------------------------------

// m survivors of the cell step: target > 0 is the reference's iterStep rule, m > target ? m / target : 1 (integer division);
// else the stride as given
EA_HD EA_SEL_INLINE int64_t select_stride_used(int64_t m, int64_t stride, int64_t target) {
  if (target > 0) return m > target ? m / target : 1;
  return stride;
}
// ordinals 0, s, 2 s, ... of m survivors
EA_HD EA_SEL_INLINE int64_t select_count_after(int64_t m, int64_t stride_used) { return (m + stride_used - 1) / stride_used; }

// ---- what the kernels are handed ------------------------------------------------------------------------------------------------

// one segment per problem of the call (its head family)
struct PointSelectSeg {
  const void *x, *y, *z;       // the stored points, n each, in the problem dtype; the weights w_in elements behind z
  void *ox, *oy, *oz;          // room for n each; the weights land w_out elements behind oz
  int64_t w_in, w_out;
  int32_t n, weighted;
  double fx, fy, cx, cy;
  int32_t height, width;       // the pixel grid of the cell step
  int32_t cells_x, pad_;
  unsigned long long *zmin;    // NEAREST: per cell the smallest bits of z; all ones before the key pass
  unsigned int *imin;          // per cell the winning point index; all ones before the key pass
  int32_t *block_counts;       // ceil(n / kPointSelectThreads) flagged-point counts, turned into offsets by the scan
};
// behind the records: the two counters of a segment the device writes
struct PointSelectOut { unsigned long long no_pixel; long long after_cells; };

}  // namespace ea
