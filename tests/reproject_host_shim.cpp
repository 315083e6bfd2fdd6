// The host half of the reprojection (edge_alignment_amd/csrc/ea_reproject.h) for the host: the 3x4 matrix of step A, the
// pose <-> matrix conversions and the check of a pose argument behind a C interface that tests/test_reproject_host.py loads
// with ctypes and holds to tests/reproject_ref.py bit for bit.  Host compiler only, no device.
#include "ea_reproject.h"

extern "C" void reproject_matrix_c(const double *b_T_a, const double *T12, const double *T12inv, double *M) {
  ea::reproject_matrix(b_T_a, T12, T12inv, M);
}

extern "C" void pose_to_matrix_c(const double *q, const double *t, double *m) { ea::pose_to_matrix(q, t, m); }

extern "C" int matrix_to_pose_c(const double *m, double *q, double *t) { return ea::matrix_to_pose(m, q, t) ? 1 : 0; }

extern "C" int reproject_pose_ok_c(const double *m) { return ea::reproject_pose_ok(m) ? 1 : 0; }

extern "C" int reproject_seg_bytes_c(void) { return (int)sizeof(ea::ReprojectSeg); }
