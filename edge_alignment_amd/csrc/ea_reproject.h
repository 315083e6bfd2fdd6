// ea_reproject.h — the host half of ea_*_reproject / ea_*_overlay and the pose <-> matrix conversions, as pure logic: shared
// by the host driver (ea_segments.hip), the kernel's work description (ea_launch.h) and a host shim without a device
// (tests/reproject_host_shim.cpp).
//
// Everything here is fp64 with a FIXED operation order and no contracted multiply-add (ea_pixel_cost_kernel's comment says
// why: one fused rounding moves a borderline pixel).  x86-64 host builds have no FMA to contract into unless asked for; the
// pragma below pins it for clang (hipcc's host pass), and the g++ shim is built with -ffp-contract=off.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__clang__)
#define EA_FP_EXACT _Pragma("clang fp contract(off)")
#else
#define EA_FP_EXACT
#endif

namespace ea {

// PoseManipUtils::raw_to_eigenmat: Eigen's Quaternion::toRotationMatrix arithmetic on q = (w, x, y, z) as given (not
// normalised), t in column 3, last row 0 0 0 1; row-major 4x4
inline void pose_to_matrix(const double q[4], const double t[3], double m[16]) {
  EA_FP_EXACT
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  m[0] = 1.0 - (tyy + tzz); m[1] = txy - twz;         m[2] = txz + twy;          m[3] = t[0];
  m[4] = txy + twz;         m[5] = 1.0 - (txx + tzz); m[6] = tyz - twx;          m[7] = t[1];
  m[8] = txz - twy;         m[9] = tyz + twx;         m[10] = 1.0 - (txx + tyy); m[11] = t[2];
  m[12] = 0.0; m[13] = 0.0; m[14] = 0.0; m[15] = 1.0;
}

// PoseManipUtils::eigenmat_to_raw: Eigen's quaternion from a rotation matrix (the trace branch, else the largest diagonal
// entry with Eigen's tie rule).  false: m33 != 1, the reference's assert( T(3,3) == 1 ).
inline bool matrix_to_pose(const double m[16], double q[4], double t[3]) {
  EA_FP_EXACT
  if (!(m[15] == 1.0)) return false;
  const double tr = (m[0] + m[5]) + m[10];
  if (tr > 0.0) {
    double s = sqrt(tr + 1.0);
    q[0] = 0.5 * s;
    s = 0.5 / s;
    q[1] = (m[9] - m[6]) * s;
    q[2] = (m[2] - m[8]) * s;
    q[3] = (m[4] - m[1]) * s;
  } else {
    int i = 0;
    if (m[5] > m[0]) i = 1;
    if (m[10] > m[5 * i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    double s = sqrt(((m[5 * i] - m[5 * j]) - m[5 * k]) + 1.0);
    q[1 + i] = 0.5 * s;
    s = 0.5 / s;
    q[0] = (m[4 * k + j] - m[4 * j + k]) * s;
    q[1 + j] = (m[4 * j + i] + m[4 * i + j]) * s;
    q[1 + k] = (m[4 * k + i] + m[4 * i + k]) * s;
  }
  t[0] = m[3]; t[1] = m[7]; t[2] = m[11];
  return true;
}

// a pose handed in as b_T_a: every entry finite and the last row exactly 0 0 0 1
inline bool reproject_pose_ok(const double m[16]) {
  for (int i = 0; i < 12; ++i)
    if (!(fabs(m[i]) <= 1.7976931348623157e308)) return false;
  return m[12] == 0.0 && m[13] == 0.0 && m[14] == 0.0 && m[15] == 1.0;
}

// c = a b for row-major 4x4: every entry ((a0 b0 + a1 b1) + a2 b2) + a3 b3, summed in k order
inline void reproject_mul4(const double a[16], const double b[16], double c[16]) {
  EA_FP_EXACT
  for (int r = 0; r < 4; ++r)
    for (int col = 0; col < 4; ++col)
      c[4 * r + col] = ((a[4 * r] * b[col] + a[4 * r + 1] * b[4 + col]) + a[4 * r + 2] * b[8 + col]) + a[4 * r + 3] * b[12 + col];
}

// Step A of ea_*_reproject: the 3x4 matrix the device applies to every point.  Plain problems (T12 == NULL): rows 0-2 of
// b_T_a.  Second camera: rows 0-2 of (T12 b_T_a) T12inv, in that association.
inline void reproject_matrix(const double b_T_a[16], const double *T12, const double *T12inv, double M[12]) {
  if (!T12 || !T12inv) {
    for (int i = 0; i < 12; ++i) M[i] = b_T_a[i];
    return;
  }
  double left[16], full[16];
  reproject_mul4(T12, b_T_a, left);
  reproject_mul4(left, T12inv, full);
  for (int i = 0; i < 12; ++i) M[i] = full[i];
}

// what the reprojection kernel walks: one segment per problem of the call (its head family)
struct ReprojectSeg {
  int64_t row;        // first (u, v) row of the segment in the output: ProblemDesc::row_begin of the term
  int32_t n, term;
  double M[12];       // step A
  unsigned char *image;  // overlay: H x W x 3 bytes, painted in place (NULL: not painted)
};
constexpr int kReprojectThreads = 256;

}  // namespace ea
