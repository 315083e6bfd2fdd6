// ea_depth_gate.h — the depth-consistency gate (ea_*_depth_gate, ea_*_set_now_depth) as pure logic: the argument checks, the
// validity and conversion of a depth sample of either kind, the projection of step B, the window scan, the classification and
// the weight.  Shared by the kernel (ea_depth_gate_kernel), the host driver (ea_segments.hip) and a host shim without a device
// (tests/depth_gate_host_shim.cpp), which holds it to tests/depth_gate_ref.py bit for bit.
// Step 3b -- a depth image at 2^shift times the DT extent (gate_scaled_pixel, depth_gate_shift) -- is held to
// tests/depth_gate_scaled_ref.py by a stand-alone host program (tests/depth_gate_scaled_host_shim.cpp).
//
// include/ea_hip.h states the arithmetic.  Everything here is fp64 in that order with no contracted multiply-add (EA_FP_EXACT,
// ea_reproject.h; the g++ shim is built with -ffp-contract=off) and IEEE divisions.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/ea_hip.h"
#include "ea_reproject.h"
#include "ea_types.h"

#if defined(__clang__)
#define EA_UNROLL _Pragma("unroll")
#else
#define EA_UNROLL
#endif
// the kernel takes the whole gate inline: a call would give it a stack
#if defined(__HIPCC__)
#define EA_INLINE __forceinline__
#else
#define EA_INLINE inline
#endif
// nothing is scheduled across it (device code only)
#if defined(__HIP_DEVICE_COMPILE__)
#define EA_SCHED_FENCE __builtin_amdgcn_sched_barrier(0);
#else
#define EA_SCHED_FENCE
#endif

namespace ea {

constexpr int kDepthGateThreads = 256;
constexpr int kDepthGateMaxRadius = 3;
constexpr int kDepthGateClasses = 6;
constexpr int kDepthGateMaxShift = 8;

// ---- argument checks (host; NULL = fine, else what is wrong) ---------------------------------------------------------------

inline bool gate_finite_nonneg(double v) { return v >= 0.0 && v <= 1.7976931348623157e308; }  // (false for NaN)

inline const char *now_depth_args_error(int kind, int height, int width, double z_scaling) {
  if (kind != EA_DEPTH_U16 && kind != EA_DEPTH_F32) return "kind must be EA_DEPTH_U16 or EA_DEPTH_F32";
  if (height < 3 || width < 3 || height > 32768 || width > 32768) return "height and width must lie in 3..32768";
  if (kind == EA_DEPTH_U16 && !(z_scaling > 0.0 && z_scaling <= 1.7976931348623157e308)) return "z_scaling must be finite and > 0";
  return nullptr;
}

inline const char *depth_gate_params_error(const ea_depth_gate_params *prm) {
  if (prm->radius < 0 || prm->radius > kDepthGateMaxRadius) return "radius must lie in 0..3";
  if (!gate_finite_nonneg(prm->abs_tol) || !gate_finite_nonneg(prm->rel_tol)) return "abs_tol and rel_tol must be finite and >= 0";
  if (!gate_finite_nonneg(prm->w_occluded) || !gate_finite_nonneg(prm->w_free) || !gate_finite_nonneg(prm->w_unknown))
    return "w_occluded, w_free and w_unknown must be finite and >= 0";
  return nullptr;
}

// the factors of an fp32 problem must be floats: wmax = FLT_MAX there, DBL_MAX otherwise
inline bool depth_gate_factors_fit(const ea_depth_gate_params *prm, double wmax) {
  return prm->w_occluded <= wmax && prm->w_free <= wmax && prm->w_unknown <= wmax;
}

// ---- what the kernel is handed -----------------------------------------------------------------------------------------------

// the rule of one call, uniform for every segment: the tolerances and the factor g of each class (1 for BEHIND, OUTSIDE,
// CONSISTENT)
struct DepthGateRule {
  double abs_tol, rel_tol;
  double g[kDepthGateClasses];
};

inline DepthGateRule depth_gate_rule(const ea_depth_gate_params *prm) {
  DepthGateRule r;
  r.abs_tol = prm->abs_tol; r.rel_tol = prm->rel_tol;
  for (int c = 0; c < kDepthGateClasses; ++c) r.g[c] = 1.0;
  r.g[EA_GATE_UNKNOWN] = prm->w_unknown; r.g[EA_GATE_OCCLUDED] = prm->w_occluded; r.g[EA_GATE_FREE] = prm->w_free;
  return r;
}

// one segment per problem of the call (its head family)
struct DepthGateSeg {
  int64_t row;          // first class byte of the segment in the rows layout: ProblemDesc::row_begin of the term
  int32_t n, term;
  double M[12];         // step A (ea_reproject.h: reproject_matrix)
  const void *depth;    // the problem's now-depth of the call's kind, (H << shift) x (W << shift), H x W the descriptor's
  double z_scaling;     // U16: metres = d / z_scaling
  void *weights;        // apply: the problem's weights behind z, in the problem dtype; NULL: nothing is written
  unsigned char *cls;   // class bytes of the segment's first point, or NULL
  double dw_z_ref;      // depth weighting of the problem (power 0: dd = 1)
  int32_t dw_power;
  int32_t shift;        // step 3b: the depth image is 2^shift times the DT extent, 0..kDepthGateMaxShift
};

// ---- a depth sample: validity and conversion -----------------------------------------------------------------------------------

// the raw value that stands for "no measurement" in both kinds: what a window pixel outside the image is read as
EA_HD EA_INLINE bool depth_sample(uint16_t raw, double z_scaling, double *d) {
  EA_FP_EXACT
  if (raw == 0) return false;
  *d = (double)raw / z_scaling;
  return true;
}
EA_HD EA_INLINE bool depth_sample(float raw, double, double *d) {
  if (!(raw > 0.0f && raw <= 3.4028234663852886e38f)) return false;  // NaN, <= 0, +Inf
  *d = (double)raw;
  return true;
}

// ---- steps 1-3: projection (step B of ea_*_reproject) and the inside rule ------------------------------------------------------

// dist: k1, k2, p1, p2, k3 by name, or NULL for the overloads without distortion
EA_HD EA_INLINE void gate_project(const double *M, double x, double y, double z, double fx, double fy, double cx, double cy,
                               const double *dist, double *bz_out, double *u, double *v) {
  EA_FP_EXACT
  const double bx = ((M[0] * x + M[1] * y) + M[2] * z) + M[3];
  const double by = ((M[4] * x + M[5] * y) + M[6] * z) + M[7];
  const double bz = ((M[8] * x + M[9] * y) + M[10] * z) + M[11];
  double xd = bx / bz, yd = by / bz;
  if (dist) {
    const double k1 = dist[0], k2 = dist[1], p1 = dist[2], p2 = dist[3], k3 = dist[4];
    const double xn = xd, yn = yd;
    const double r2 = xn * xn + yn * yn, r4 = r2 * r2, r6 = r4 * r2;
    const double rad = ((1.0 + k1 * r2) + k2 * r4) + k3 * r6;
    xd = (xn * rad + ((2.0 * p1) * xn) * yn) + p2 * (r2 + (2.0 * xn) * xn);
    yd = (yn * rad + ((2.0 * p2) * xn) * yn) + p1 * (r2 + (2.0 * yn) * yn);
  }
  *bz_out = bz;
  *u = fx * xd + cx;
  *v = fy * yd + cy;
}

EA_HD EA_INLINE bool gate_behind(double bz) { return !(bz > 0.0 && bz <= 1.7976931348623157e308); }  // NaN included

// ea_problem_pixel_cost's rule (the `inside` test of ea_reproject_kernel); iu, iv: the truncated pixel when inside
EA_HD EA_INLINE bool gate_inside(double u, double v, int H, int W, int *iu_out, int *iv_out) {
  const bool finite = (u == u) && (v == v) && fabs(u) < 1e9 && fabs(v) < 1e9;
  const int iu = finite ? (int)u : -1, iv = finite ? (int)v : -1;  // `(int)`: truncation toward zero
  *iu_out = iu; *iv_out = iv;
  return finite && iu >= 0 && iu < W && iv >= 0 && iv < H && !(u <= -1.0) && !(v <= -1.0);
}

// step 3b: the pixel of a depth image at 2^shift times the DT extent under the inside point (u, v).  c = (2^shift - 1) / 2 is
// the centre of the 2^shift x 2^shift block of depth pixels whose mean DT pixel 0 is (exact); u * 2^shift is exact, the
// addition rounds once.  shift = 0: U = u.  (u, v) inside: |U| < 2^31 for every extent the host accepts.
EA_HD EA_INLINE void gate_scaled_pixel(double u, double v, int shift, int *iu_out, int *iv_out) {
  EA_FP_EXACT
  const double scale = (double)(1 << shift), c = (scale - 1.0) * 0.5;
  const double U = u * scale + c, V = v * scale + c;
  *iu_out = (int)U; *iv_out = (int)V;
}

// the shift s with (nd_H, nd_W) == (H << s, W << s) and H * W << 2 s <= 2^30, or -1 (host: the extent rule of ea_*_depth_gate)
inline int depth_gate_shift(int H, int W, int nd_H, int nd_W) {
  for (int s = 0; s <= kDepthGateMaxShift; ++s) {
    if (((int64_t)H * W) << (2 * s) > ((int64_t)1 << 30)) break;
    if (((int64_t)H << s) == nd_H && ((int64_t)W << s) == nd_W) return s;
  }
  return -1;
}

// ---- steps 4-5: the window scan and the classification --------------------------------------------------------------------------

// a raw sample kept (keep = ~0) or turned into 0, the "no measurement" of both kinds (keep = 0), by integer arithmetic: a lane
// mask per window pixel would occupy a scalar register pair each until its load has landed
EA_HD EA_INLINE uint16_t gate_keep(uint16_t raw, int keep) { return (uint16_t)(raw & (unsigned)keep); }
EA_HD EA_INLINE float gate_keep(float raw, int keep) {
  unsigned bits;
  memcpy(&bits, &raw, sizeof(bits));
  bits &= (unsigned)keep;
  memcpy(&raw, &bits, sizeof(bits));
  return raw;
}

// The (2 R + 1)^2 pixels around (iv, iu), dy outer and dx inner: all loads first -- independent of each other, a pixel outside
// the image reads pixel 0 and becomes 0, "no measurement" in both kinds -- then the compare chain: the first valid pixel, and
// any later one with a strictly smaller |d - bz|.  false: no valid pixel.  (EA_SCHED_FENCE: the chain is taken a window row
// at a time on the device, or the scheduler converts and divides all 49 samples at once and runs out of registers.)
template <typename RAW, int R, typename PTR = const RAW *>  // (PTR: the kernel reads through a global-address-space pointer)
EA_HD EA_INLINE bool gate_scan(PTR img, int H, int W, int iu, int iv, double z_scaling, double bz, double *d_best) {
  EA_FP_EXACT
  constexpr int S = 2 * R + 1;
  RAW raw[S * S];
EA_UNROLL
  for (int dy = -R; dy <= R; ++dy) {
EA_UNROLL
    for (int dx = -R; dx <= R; ++dx) {
      const int row = iv + dy, col = iu + dx;
      const int outside = (row | col | (H - 1 - row) | (W - 1 - col)) >> 31;  // all ones when a coordinate is out of range
      const int at = (row * W + col) & ~outside;                             // (H x W <= 2^30; pixel 0 can always be read)
      const RAW val = img[at];
      raw[(dy + R) * S + (dx + R)] = gate_keep(val, ~outside);
    }
  }
  bool have = false;
  double best = 0.0, best_e = 0.0;
EA_UNROLL
  for (int r = 0; r < S; ++r) {
    EA_SCHED_FENCE
EA_UNROLL
    for (int c = 0; c < S; ++c) {
      double d;
      if (depth_sample(raw[r * S + c], z_scaling, &d)) {
        const double e = fabs(d - bz);
        if (!have || e < best_e) { best = d; best_e = e; have = true; }
      }
    }
  }
  *d_best = best;
  return have;
}

// the radius as a run-time value, for the host
template <typename RAW>
inline bool gate_scan_radius(int radius, const RAW *img, int H, int W, int iu, int iv, double z_scaling, double bz, double *d_best) {
  switch (radius) {
    case 0: return gate_scan<RAW, 0>(img, H, W, iu, iv, z_scaling, bz, d_best);
    case 1: return gate_scan<RAW, 1>(img, H, W, iu, iv, z_scaling, bz, d_best);
    case 2: return gate_scan<RAW, 2>(img, H, W, iu, iv, z_scaling, bz, d_best);
    default: return gate_scan<RAW, 3>(img, H, W, iu, iv, z_scaling, bz, d_best);
  }
}

EA_HD EA_INLINE int gate_classify(double d, double bz, double abs_tol, double rel_tol) {
  EA_FP_EXACT
  const double tol = abs_tol + rel_tol * bz;
  const double diff = d - bz;
  if (fabs(diff) <= tol) return EA_GATE_CONSISTENT;
  return diff < 0.0 ? EA_GATE_OCCLUDED : EA_GATE_FREE;
}

// steps 1-5 for one point; H x W: the DT extent, img: (H << shift) x (W << shift)
template <typename RAW, int R, typename PTR = const RAW *>
EA_HD EA_INLINE int gate_point(const double *M, double x, double y, double z, double fx, double fy, double cx, double cy,
                            const double *dist, PTR img, int H, int W, double z_scaling, double abs_tol,
                            double rel_tol, int shift = 0) {
  double bz, u, v;
  gate_project(M, x, y, z, fx, fy, cx, cy, dist, &bz, &u, &v);
  if (gate_behind(bz)) return EA_GATE_BEHIND;
  int iu, iv;
  if (!gate_inside(u, v, H, W, &iu, &iv)) return EA_GATE_OUTSIDE;
  gate_scaled_pixel(u, v, shift, &iu, &iv);
  double d;
  if (!gate_scan<RAW, R, PTR>(img, H << shift, W << shift, iu, iv, z_scaling, bz, &d)) return EA_GATE_UNKNOWN;
  return gate_classify(d, bz, abs_tol, rel_tol);
}

// ---- step 6 and the weight -------------------------------------------------------------------------------------------------------

// dd: min(1, (z_ref / z)^power) as depth_weights_body (ea_kernels.hip) forms it before its rounding -- one division, power - 1
// multiplications left to right, the clamp to [0, 1]; power <= 0: 1
EA_HD EA_INLINE double gate_depth_factor(double z, double z_ref, int power) {
  EA_FP_EXACT
  if (power <= 0) return 1.0;
  const double ratio = z_ref / z;
  double v = ratio;
  for (int k = 1; k < power; ++k) v = v * ratio;
  return fmax(0.0, fmin(1.0, v));
}

// step 6: the factor of a class, by selects (the rule is uniform: no indexed read of it)
EA_HD EA_INLINE double gate_factor(const DepthGateRule &rule, int cls) {
  return cls == EA_GATE_UNKNOWN ? rule.g[EA_GATE_UNKNOWN]
         : cls == EA_GATE_OCCLUDED ? rule.g[EA_GATE_OCCLUDED]
         : cls == EA_GATE_FREE ? rule.g[EA_GATE_FREE] : 1.0;
}

// w = g * dd, one multiplication; the caller rounds it once to the problem dtype
EA_HD EA_INLINE double gate_weight(double g, double dd) {
  EA_FP_EXACT
  return g * dd;
}

}  // namespace ea
