// Host shim for tests/test_point_select_host.py: edge_alignment_amd/csrc/ea_point_select.h compiled with the host compiler
// (-ffp-contract=off), so the rule the kernels run is checked against tests/point_select_ref.py without a device.
#include <stdint.h>

#include "ea_point_select.h"

extern "C" {

// xyz: n x 3 doubles as stored.  has / pu / pv: per point; cell: the cell with cell_px > 0 (0 without a pixel or a cell step)
void point_select_pixels_c(const double *xyz, int64_t n, double fx, double fy, double cx, double cy, int height, int width,
                           int cell_px, int *has, int *pu, int *pv, int64_t *cell) {
  const int cells_x = cell_px > 0 ? ea::select_cells_x(cell_px, width) : 0;
  for (int64_t i = 0; i < n; ++i) {
    has[i] = ea::select_pixel(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], fx, fy, cx, cy, height, width, &pu[i], &pv[i]) ? 1 : 0;
    cell[i] = has[i] && cell_px > 0 ? ea::select_cell(pu[i], pv[i], cell_px, cells_x) : 0;
  }
}

int64_t point_select_stride_used_c(int64_t m, int64_t stride, int64_t target) { return ea::select_stride_used(m, stride, target); }
int64_t point_select_count_after_c(int64_t m, int64_t stride_used) { return ea::select_count_after(m, stride_used); }
int64_t point_selection_cells_c(int cell_px, int height, int width) { return ea::point_selection_cells(cell_px, height, width); }

int point_selection_ok_c(int cell_px, int cell_rule, int outside, int height, int width, int64_t stride, int64_t target) {
  ea_point_selection prm;
  prm.cell_px = cell_px; prm.cell_rule = cell_rule; prm.outside = outside; prm.height = height; prm.width = width;
  prm.stride = stride; prm.target = target;
  return ea::point_selection_ok(&prm) ? 1 : 0;
}

int point_selection_is_identity_c(int cell_px, int64_t stride, int64_t target) {
  ea_point_selection prm = {};
  prm.cell_px = cell_px; prm.stride = stride; prm.target = target;
  return ea::point_selection_is_identity(&prm) ? 1 : 0;
}

int point_select_seg_bytes_c(void) { return (int)sizeof(ea::PointSelectSeg); }
int point_select_out_bytes_c(void) { return (int)sizeof(ea::PointSelectOut); }
}
