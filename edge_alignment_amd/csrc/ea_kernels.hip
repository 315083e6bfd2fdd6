// ea_kernels.hip — gfx950 (MI355X / CDNA4) kernels of the edge-alignment hot path.
//
// What the reference does per edge point on one CPU thread with dual numbers
// (ref: standalone/utils.h:48-80 EAResidue::operator(), ceres BiCubicInterpolator, AutoDiff,
// QuaternionParameterization, loss corrector) is done here by one lane per point:
//   b = R a + t  ->  (u,v) = K b / b_z  ->  16-tap Catmull-Rom sample of the DT image with
//   analytic d/du, d/dv  ->  analytic 1x6 row  ->  IRLS weight  ->  28 fp64 accumulators,
// followed by a wavefront-level transposing butterfly and a fixed-order cross-wave / cross-tile
// reduction (bit-reproducible: no float atomics).
//
// Data layout in HBM: points as SoA x[],y[],z[] (coalesced 4/8-byte loads per lane); the DT
// image row-major [v][u] with a 3-texel replicated border so that Grid2D's clamp-to-edge
// addressing needs no per-tap clamps; per-tile partial sums as 32 doubles (256 B) per tile.
// A workgroup handles a tile = run of consecutive points; their projected footprint (+halo) is
// staged through LDS when it fits, otherwise the taps come from L2 directly (four unaligned
// 16-byte row loads per point).
//
// No MFMA: pointwise arithmetic plus a 28-value reduction.

#include <hip/hip_runtime.h>

#include <cstddef>
#include <type_traits>

#if defined(EA_STAMPS) && defined(__HIP_DEVICE_COMPILE__)
namespace ea {
extern __device__ unsigned long long *g_lm_stamp_buf;
extern __device__ int g_lm_probe_row;
}
#define EA_LM_PROBE(k)                                                                              \
  do {                                                                                              \
    if (g_lm_stamp_buf && blockIdx.x == 0) {                                                        \
      unsigned long long t_;                                                                        \
      __builtin_amdgcn_sched_barrier(0);                                                            \
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                    \
      __builtin_amdgcn_sched_barrier(0);                                                            \
      g_lm_stamp_buf[64 * 8 + g_lm_probe_row * 8 + (k)] = t_;                                       \
    }                                                                                               \
  } while (0)
#endif
#include "ea_lanes_stream.h"
#include "ea_launch.h"
#include "ea_poses_map.h"
#include "ea_starts_map.h"
#include "ea_depth_gate.h"
#include "ea_point_select.h"
#include "ea_point_merge.h"
#include "ea_lm.h"
#include "ea_pair_log.h"
#include "ea_prior.h"
#include "ea_reproject.h"
#include "ea_select.h"
#include "ea_types.h"
#include "ea_wave_exchange.h"

namespace ea {

// Diagnostic build only (-DEA_STAMPS, scripts/build_stamps.sh -> lib/libea_hip_stamps.so): wave 0 of every
// workgroup stamps s_memtime at the phase boundaries into a buffer of its own; no output value depends on it.
#ifdef EA_STAMPS
__device__ unsigned long long *g_stamp_buf = nullptr;
#ifndef EA_STAMPS_EVAL
// (the evaluation kernel's stamps need -DEA_STAMPS_EVAL on top: since the kernel head keeps its uniforms in named SGPRs the
// stamped form of it no longer compiles on this toolchain -- "illegal VGPR to SGPR copy"; the LM-step stamps are unaffected)
#define EA_STAMP(slot) do {} while (0)
#else
#define EA_STAMP(slot)                                                                              \
  do {                                                                                              \
    if (g_stamp_buf && threadIdx.x == 0) {                                                          \
      unsigned long long t_;                                                                        \
      __builtin_amdgcn_sched_barrier(0);                                                            \
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                    \
      __builtin_amdgcn_sched_barrier(0);                                                            \
      g_stamp_buf[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 8 + (slot)] = t_;                 \
    }                                                                                               \
  } while (0)
#endif
__device__ unsigned long long *g_lm_stamp_buf = nullptr;  // [64 evaluations][8] kernel + [64][8] state-machine probes, problem 0
__device__ int g_lm_probe_row = 0;
#define EA_LM_STAMP(slot, eval)                                                                     \
  do {                                                                                              \
    if (g_lm_stamp_buf && threadIdx.x == 0 && blockIdx.x == 0) {                                    \
      unsigned long long t_;                                                                        \
      __builtin_amdgcn_sched_barrier(0);                                                            \
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                    \
      __builtin_amdgcn_sched_barrier(0);                                                            \
      g_lm_stamp_buf[((eval) & 63) * 8 + (slot)] = t_;                                              \
    }                                                                                               \
  } while (0)
// (a stamp taken before its row index is known: read the clock now, store later)
#define EA_LM_CLOCK(var)                                                                            \
  unsigned long long var = 0;                                                                       \
  do {                                                                                              \
    __builtin_amdgcn_sched_barrier(0);                                                              \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(var)::"memory");                    \
    __builtin_amdgcn_sched_barrier(0);                                                              \
  } while (0)
#define EA_LM_STAMP_PUT(slot, eval, var)                                                            \
  do {                                                                                              \
    if (g_lm_stamp_buf && threadIdx.x == 0 && blockIdx.x == 0) g_lm_stamp_buf[((eval) & 63) * 8 + (slot)] = var; \
  } while (0)
#else
#define EA_STAMP(slot) do {} while (0)
#define EA_LM_STAMP(slot, eval) do {} while (0)
#define EA_LM_CLOCK(var) do {} while (0)
#define EA_LM_STAMP_PUT(slot, eval, var) do {} while (0)
#endif

// ------------------------------------------------------------------------------------------------
// arithmetic helpers, T = float | double

template <typename T> __device__ __forceinline__ T t_rcp(T x);
template <> __device__ __forceinline__ float t_rcp<float>(float x) { return __builtin_amdgcn_rcpf(x); }
// v_rcp_f64 + two Newton steps: 5 instructions and <= 1 ulp instead of the ~14 of an IEEE division (three per point)
template <> __device__ __forceinline__ double t_rcp<double>(double x) {
  double r = __builtin_amdgcn_rcp(x);
  double e = __builtin_fma(-x, r, 1.0);
  r = __builtin_fma(r, e, r);
  e = __builtin_fma(-x, r, 1.0);
  return __builtin_fma(r, e, r);
}

template <typename T> __device__ __forceinline__ T t_log(T x);
// v_log_f32 is log2 and needs no denormal pre-scaling here: its only caller passes 1 + s / a^2 >= 1
template <> __device__ __forceinline__ float t_log<float>(float x) { return __builtin_amdgcn_logf(x) * 0.6931471805599453f; }

// A floating-point literal as a scalar-register operand.  VOP3 takes no 64-bit literal on gfx950: left alone, the compiler
// rebuilds such a constant in a VGPR pair (two v_mov_b32) in front of every v_fma_f64 that uses it; through an "s" operand
// it is two s_mov_b32 on the scalar port and the fma reads the pair directly.  (One scalar operand per VALU instruction:
// where an expression has two literals, only one of them goes through here.)
__device__ __forceinline__ double s_const(double c) { asm("" : "+s"(c)); return c; }
__device__ __forceinline__ float s_const(float c) { return c; }  // (fp32 literals are operands already)

// fp64 log for the Cauchy loss (ea_pair_log.h), argument 1 + s / a^2 in [1, inf): frexp to m in [sqrt(1/2), sqrt(2)), then
// log m = 2 atanh z as the odd series to z^21.  ~33 instructions and ~2 ulp, against ~110 for libm's log.
struct LogOps {
  static __device__ __forceinline__ double frexp_mant(double x) { return __builtin_amdgcn_frexp_mant(x); }
  static __device__ __forceinline__ int frexp_exp(double x) { return __builtin_amdgcn_frexp_exp(x); }
  static __device__ __forceinline__ double ldexp(double x, int e) { return __builtin_amdgcn_ldexp(x, e); }
  static __device__ __forceinline__ double rcp(double x) { return __builtin_amdgcn_rcp(x); }
  static __device__ __forceinline__ double sconst(double c) { return s_const(c); }
};
template <> __device__ __forceinline__ double t_log<double>(double x) { return pl_log<LogOps>(x); }

template <typename T> __device__ __forceinline__ T t_sqrt(T x);
template <> __device__ __forceinline__ float t_sqrt<float>(float x) { return __builtin_amdgcn_sqrtf(x); }
template <> __device__ __forceinline__ double t_sqrt<double>(double x) { return sqrt(x); }

template <typename T> __device__ __forceinline__ T t_fma(T a, T b, T c) { return __builtin_fma(a, b, c); }
template <> __device__ __forceinline__ float t_fma<float>(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

// Catmull-Rom weights of the four taps at fraction x, and their derivatives
// (ceres CubicHermiteSpline written as tap weights).  fp64: 1.5 and 4.5 are scalar operands (s_const); -2.5 and -5 share an
// fma with one of them and stay vector literals.
template <typename T>
__device__ __forceinline__ void cr_weights(T x, T w[4], T d[4]) {
  const T x2 = x * x;
  const T c15 = s_const(T(1.5));
  w[0] = x * t_fma<T>(x, t_fma<T>(T(-0.5), x, T(1)), T(-0.5));
  w[1] = t_fma<T>(x2, t_fma<T>(c15, x, T(-2.5)), T(1));
  w[2] = x * t_fma<T>(x, t_fma<T>(-c15, x, T(2)), T(0.5));
  w[3] = x2 * t_fma<T>(T(0.5), x, T(-0.5));
  const T c45 = s_const(T(4.5));
  d[0] = t_fma<T>(x, t_fma<T>(-c15, x, T(2)), T(-0.5));
  d[1] = x * t_fma<T>(c45, x, T(-5));
  d[2] = t_fma<T>(x, t_fma<T>(-c45, x, T(4)), T(0.5));
  d[3] = x * t_fma<T>(c15, x, T(-1));
}

// uniform (per-problem / per-pose) values in the kernel's arithmetic type
template <typename T> struct Uni;
template <> struct Uni<double> {
  static __device__ __forceinline__ const double *R(const PoseState &ps) { return ps.R; }
  static __device__ __forceinline__ const double *t(const PoseState &ps) { return ps.t; }
  static __device__ __forceinline__ const double *G(const PoseState &ps) { return ps.G; }
  static __device__ __forceinline__ double fx(const ProblemDesc &pd) { return pd.fx; }
  static __device__ __forceinline__ double fy(const ProblemDesc &pd) { return pd.fy; }
  static __device__ __forceinline__ double cx(const ProblemDesc &pd) { return pd.cx; }
  static __device__ __forceinline__ double cy(const ProblemDesc &pd) { return pd.cy; }
  static __device__ __forceinline__ double loss_a(const ProblemDesc &pd) { return pd.loss_a; }
  static __device__ __forceinline__ double loss_inv_b(const ProblemDesc &pd) { return pd.loss_inv_b; }
  static __device__ __forceinline__ double z_guard(const ProblemDesc &pd) { return pd.z_guard; }
  static __device__ __forceinline__ double z_eps(const ProblemDesc &pd) { return pd.z_eps; }
  static __device__ __forceinline__ const double *dist(const ProblemDesc &pd) { return pd.dist; }
  static __device__ __forceinline__ const double *A(const ProblemDesc &pd) { return pd.A; }
  static __device__ __forceinline__ const double *d(const ProblemDesc &pd) { return pd.d; }
  static __device__ __forceinline__ const double *Ai(const ProblemDesc &pd) { return pd.Ai; }
  static __device__ __forceinline__ const double *di(const ProblemDesc &pd) { return pd.di; }
};
template <> struct Uni<float> {
  static __device__ __forceinline__ const float *R(const PoseState &ps) { return ps.Rf; }
  static __device__ __forceinline__ const float *t(const PoseState &ps) { return ps.tf; }
  static __device__ __forceinline__ const float *G(const PoseState &ps) { return ps.Gf; }
  static __device__ __forceinline__ float fx(const ProblemDesc &pd) { return pd.fxf; }
  static __device__ __forceinline__ float fy(const ProblemDesc &pd) { return pd.fyf; }
  static __device__ __forceinline__ float cx(const ProblemDesc &pd) { return pd.cxf; }
  static __device__ __forceinline__ float cy(const ProblemDesc &pd) { return pd.cyf; }
  static __device__ __forceinline__ float loss_a(const ProblemDesc &pd) { return pd.loss_af; }
  static __device__ __forceinline__ float loss_inv_b(const ProblemDesc &pd) { return pd.loss_inv_bf; }
  static __device__ __forceinline__ float z_guard(const ProblemDesc &pd) { return pd.z_guardf; }
  static __device__ __forceinline__ float z_eps(const ProblemDesc &pd) { return pd.z_epsf; }
  static __device__ __forceinline__ const float *dist(const ProblemDesc &pd) { return pd.distf; }
  static __device__ __forceinline__ const float *A(const ProblemDesc &pd) { return pd.Af; }
  static __device__ __forceinline__ const float *d(const ProblemDesc &pd) { return pd.df; }
  static __device__ __forceinline__ const float *Ai(const ProblemDesc &pd) { return pd.Aif; }
  static __device__ __forceinline__ const float *di(const ProblemDesc &pd) { return pd.dif; }
};

// The pose as the fused kernel carries it: rotation and translation in the kernel's arithmetic type, held in SGPRs
// (fetched speculatively in the same batch as the descriptor), the rarely needed rest through a pointer.
template <typename T>
struct PoseLite {
  T R[9], t[3];
  int unit_q;
  const PoseState *full;
};
template <typename T> struct PoseAcc {
  static __device__ __forceinline__ const T *R(const PoseState &ps) { return Uni<T>::R(ps); }
  static __device__ __forceinline__ const T *t(const PoseState &ps) { return Uni<T>::t(ps); }
  static __device__ __forceinline__ const T *G(const PoseState &ps) { return Uni<T>::G(ps); }
  static __device__ __forceinline__ int unit_q(const PoseState &ps) { return ps.unit_q; }
  static __device__ __forceinline__ const T *R(const PoseLite<T> &ps) { return ps.R; }
  static __device__ __forceinline__ const T *t(const PoseLite<T> &ps) { return ps.t; }
  static __device__ __forceinline__ const T *G(const PoseLite<T> &ps) { return Uni<T>::G(*ps.full); }
  static __device__ __forceinline__ int unit_q(const PoseLite<T> &ps) { return ps.unit_q; }
};

// per-point state carried from the projection phase to the sampling phase
template <typename T>
struct Proj {
  T bx, by, iz;    // warped point (x, y) and 1 / (b_z + z_eps)
  T fxz, fyz;      // fx * iz, fy * iz
  T cx_, cy_, cz_; // R a  (= b - t), for the unit-quaternion Jacobian
  T fu, fv;        // fractional parts of (u, v)
  int iu, iv;      // floor(u), floor(v), saturated to [-2, W] / [-2, H]
  int state;       // 0 = lane has no point, 1 = valid, 2 = functor returned false
  T u, v;          // the projection itself (read by ea_pose_stats_kernel alone; dead, and dropped, in every other kernel)
};

template <typename T, typename PS>
__device__ __forceinline__ void project_point(const ProblemDesc &pd, const PS &ps, T x, T y, T z,
                                              Proj<T> &o) {
  const T *R = PoseAcc<T>::R(ps);
  const T *t = PoseAcc<T>::t(ps);
  const T cxr = t_fma<T>(R[2], z, t_fma<T>(R[1], y, R[0] * x));
  const T cyr = t_fma<T>(R[5], z, t_fma<T>(R[4], y, R[3] * x));
  const T czr = t_fma<T>(R[8], z, t_fma<T>(R[7], y, R[6] * x));
  const T bx = cxr + t[0], by = cyr + t[1], bz = czr + t[2];
  const T zg = Uni<T>::z_guard(pd);
  // ref: utils.h:70-73 — `return false` inside (-0.01, 0.01)
  const bool bad = (zg > T(0)) && (bz < zg) && (bz > -zg);
  const T iz = t_rcp<T>(bz + Uni<T>::z_eps(pd));
  // fx / b_z and fy / b_z serve the projection here and the gradient in jacobian_row
  const T fxz = Uni<T>::fx(pd) * iz, fyz = Uni<T>::fy(pd) * iz;
  const T u = t_fma<T>(fxz, bx, Uni<T>::cx(pd));
  const T v = t_fma<T>(fyz, by, Uni<T>::cy(pd));
  // Texel index saturates: beyond [-2, W] x [-2, H] every tap is the replicated border texel.
  // The fraction stays the true one (Ceres: r - int(floor(r))): with equal taps the spline is
  // constant only while the weights stay O(1).
  const T uf = floor(u), vf = floor(v);
  o.bx = bx; o.by = by; o.iz = iz;
  o.fxz = fxz; o.fyz = fyz;
  o.cx_ = cxr; o.cy_ = cyr; o.cz_ = czr;
  o.fu = u - uf;
  o.fv = v - vf;
  o.iu = (int)fmin(fmax(uf, T(-2)), (T)pd.W);
  o.iv = (int)fmin(fmax(vf, T(-2)), (T)pd.H);
  o.state = bad ? 2 : 1;
  o.u = u; o.v = v;
}

// ---- residual variants: EAResidueEx (Brown-Conrady distortion, utils.h:102-177),
// EAResidueSecondCam (second camera of a rigid rig, b_T_a' = T12 b_T_a T12^-1, utils.h:179-292) and both
// (utils.h:295-421).  Same skeleton as the plain functor with an affine map either side of the pose and the
// distortion chain rule in the gradient.
template <typename T>
struct ProjV {
  T x, y, iz;       // normalised image coordinates and 1 / (b_z + z_eps)
  T ax, ay, az;     // a' = T12^-1 a (the point the pose acts on)
  T cx_, cy_, cz_;  // R a'
  T xdx, xdy, ydx, ydy;  // d(distorted x,y) / d(x,y)
  T fu, fv;
  int iu, iv;
  int state;
  T u, v;           // as Proj's
};

template <typename T, typename PS>
__device__ __forceinline__ void project_point_var(const ProblemDesc &pd, const PS &ps, T px, T py, T pz,
                                                  ProjV<T> &o) {
  const T *R = PoseAcc<T>::R(ps);
  const T *t = PoseAcc<T>::t(ps);
  T ax = px, ay = py, az = pz;
  if (pd.variant & 2) {
    const T *Ai = Uni<T>::Ai(pd), *di = Uni<T>::di(pd);
    ax = t_fma<T>(Ai[2], pz, t_fma<T>(Ai[1], py, Ai[0] * px)) + di[0];
    ay = t_fma<T>(Ai[5], pz, t_fma<T>(Ai[4], py, Ai[3] * px)) + di[1];
    az = t_fma<T>(Ai[8], pz, t_fma<T>(Ai[7], py, Ai[6] * px)) + di[2];
  }
  const T cxr = t_fma<T>(R[2], az, t_fma<T>(R[1], ay, R[0] * ax));
  const T cyr = t_fma<T>(R[5], az, t_fma<T>(R[4], ay, R[3] * ax));
  const T czr = t_fma<T>(R[8], az, t_fma<T>(R[7], ay, R[6] * ax));
  T bx = cxr + t[0], by = cyr + t[1], bz = czr + t[2];
  if (pd.variant & 2) {
    const T *A = Uni<T>::A(pd), *d = Uni<T>::d(pd);
    const T c0 = bx, c1 = by, c2 = bz;
    bx = t_fma<T>(A[2], c2, t_fma<T>(A[1], c1, A[0] * c0)) + d[0];
    by = t_fma<T>(A[5], c2, t_fma<T>(A[4], c1, A[3] * c0)) + d[1];
    bz = t_fma<T>(A[8], c2, t_fma<T>(A[7], c1, A[6] * c0)) + d[2];
  }
  const T zg = Uni<T>::z_guard(pd);
  const bool bad = (zg > T(0)) && (bz < zg) && (bz > -zg);
  const T iz = t_rcp<T>(bz + Uni<T>::z_eps(pd));
  const T x = bx * iz, y = by * iz;
  T xd = x, yd = y;
  o.xdx = T(1); o.xdy = T(0); o.ydx = T(0); o.ydy = T(1);
  if (pd.variant & 1) {
    const T *k = Uni<T>::dist(pd);  // k1, k2, p1, p2, k3
    const T r2 = t_fma<T>(x, x, y * y), r4 = r2 * r2, r6 = r4 * r2;
    const T D = t_fma<T>(k[4], r6, t_fma<T>(k[1], r4, t_fma<T>(k[0], r2, T(1))));
    const T Dp = t_fma<T>(T(3) * k[4], r4, t_fma<T>(T(2) * k[1], r2, k[0]));
    const T xy = x * y;
    xd = t_fma<T>(k[3], t_fma<T>(T(2) * x, x, r2), t_fma<T>(T(2) * k[2], xy, x * D));
    yd = t_fma<T>(k[2], t_fma<T>(T(2) * y, y, r2), t_fma<T>(T(2) * k[3], xy, y * D));
    o.xdx = t_fma<T>(T(6) * k[3], x, t_fma<T>(T(2) * k[2], y, t_fma<T>(T(2) * x * x, Dp, D)));
    o.xdy = t_fma<T>(T(2) * k[3], y, t_fma<T>(T(2) * k[2], x, T(2) * xy * Dp));
    o.ydx = t_fma<T>(T(2) * k[2], x, t_fma<T>(T(2) * k[3], y, T(2) * xy * Dp));
    o.ydy = t_fma<T>(T(6) * k[2], y, t_fma<T>(T(2) * k[3], x, t_fma<T>(T(2) * y * y, Dp, D)));
  }
  const T u = t_fma<T>(Uni<T>::fx(pd), xd, Uni<T>::cx(pd));
  const T v = t_fma<T>(Uni<T>::fy(pd), yd, Uni<T>::cy(pd));
  const T uf = floor(u), vf = floor(v);
  o.x = x; o.y = y; o.iz = iz;
  o.ax = ax; o.ay = ay; o.az = az;
  o.cx_ = cxr; o.cy_ = cyr; o.cz_ = czr;
  // Where the four taps along an axis are the one replicated border texel (floor <= -2 or >= extent), Ceres' Horner
  // spline returns that texel and a derivative of exactly 0.  The tap-weight form used here returns texel * (sum of the
  // derivative weights) = texel * O(eps) instead, which the distortion chain rule then multiplies by d(u,v)/d(x,y):
  // unbounded for points far outside the field of view (r^6 terms; 1e6 .. 1e12 seen in scripts/soak_variants.py, i.e.
  // rows of O(1..10) where the reference has zeros).  A zero fraction makes the weights (0,1,0,0) / (-.5,0,.5,0) and
  // both results exact.  (The plain functor's chain factor is fx / b_z <= fx / z_guard, so it keeps the true fraction.)
  o.fu = (uf <= T(-2) || uf >= (T)pd.W) ? T(0) : u - uf;
  o.fv = (vf <= T(-2) || vf >= (T)pd.H) ? T(0) : v - vf;
  o.iu = (int)fmin(fmax(uf, T(-2)), (T)pd.W);
  o.iv = (int)fmin(fmax(vf, T(-2)), (T)pd.H);
  o.state = bad ? 2 : 1;
  o.u = u; o.v = v;
}

template <typename T, typename PS>
__device__ __forceinline__ void jacobian_row_var(const ProblemDesc &pd, const PS &ps, const ProjV<T> &pr,
                                                 T Fu, T Fv, T J[6]) {
  const T fu_ = Fu * Uni<T>::fx(pd), fv_ = Fv * Uni<T>::fy(pd);
  const T rx = t_fma<T>(fv_, pr.ydx, fu_ * pr.xdx);  // d r / d x
  const T ry = t_fma<T>(fv_, pr.ydy, fu_ * pr.xdy);  // d r / d y
  T gx = rx * pr.iz, gy = ry * pr.iz, gz = -t_fma<T>(rx, pr.x, ry * pr.y) * pr.iz;  // d r / d b
  if (pd.variant & 2) {  // back through b = A c + d:  g_c = A^T g_b
    const T *A = Uni<T>::A(pd);
    const T g0 = t_fma<T>(A[6], gz, t_fma<T>(A[3], gy, A[0] * gx));
    const T g1 = t_fma<T>(A[7], gz, t_fma<T>(A[4], gy, A[1] * gx));
    const T g2 = t_fma<T>(A[8], gz, t_fma<T>(A[5], gy, A[2] * gx));
    gx = g0; gy = g1; gz = g2;
  }
  if (PoseAcc<T>::unit_q(ps)) {
    J[0] = T(2) * t_fma<T>(pr.cy_, gz, -(pr.cz_ * gy));
    J[1] = T(2) * t_fma<T>(pr.cz_, gx, -(pr.cx_ * gz));
    J[2] = T(2) * t_fma<T>(pr.cx_, gy, -(pr.cy_ * gx));
  } else {
    // (the empty asm keeps this uniform branch a branch: left alone, the compiler computes the 30 extra FMAs of the
    // general path for every point and selects afterwards)
    asm volatile("" ::: "memory");
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const T *G = PoseAcc<T>::G(ps) + 9 * j;
      const T d0 = t_fma<T>(G[2], pr.az, t_fma<T>(G[1], pr.ay, G[0] * pr.ax));
      const T d1 = t_fma<T>(G[5], pr.az, t_fma<T>(G[4], pr.ay, G[3] * pr.ax));
      const T d2 = t_fma<T>(G[8], pr.az, t_fma<T>(G[7], pr.ay, G[6] * pr.ax));
      J[j] = t_fma<T>(gz, d2, t_fma<T>(gy, d1, gx * d0));
    }
  }
  J[3] = gx; J[4] = gy; J[5] = gz;
}

// four consecutive texels of one image row; 4/8-byte aligned only (the hardware's unaligned
// access mode turns this into one or two dwordx4 loads instead of four scalar ones)
template <typename T>
struct __attribute__((packed, aligned(sizeof(T)))) Row4 {
  T p0, p1, p2, p3;
};

// 16 taps -> value and gradient.  row(l) = DT(v = iv-1+l, u = iu-1 .. iu+2)
template <typename T, typename RowFn>
__device__ __forceinline__ void bicubic(T fu, T fv, RowFn row, T &f, T &Fu, T &Fv) {
  T wu[4], du[4], wv[4], dv[4];
  cr_weights<T>(fu, wu, du);
  cr_weights<T>(fv, wv, dv);
  f = T(0); Fu = T(0); Fv = T(0);
#pragma unroll
  for (int l = 0; l < 4; ++l) {
    const Row4<T> r = row(l);
    const T rs = t_fma<T>(wu[3], r.p3, t_fma<T>(wu[2], r.p2, t_fma<T>(wu[1], r.p1, wu[0] * r.p0)));
    const T rd = t_fma<T>(du[3], r.p3, t_fma<T>(du[2], r.p2, t_fma<T>(du[1], r.p1, du[0] * r.p0)));
    f = t_fma<T>(wv[l], rs, f);
    Fv = t_fma<T>(dv[l], rs, Fv);
    Fu = t_fma<T>(wv[l], rd, Fu);
  }
}

// rho(s), rho'(s) — ceres loss_function.cc
// log(1 + x), x >= 0, as the Cauchy loss needs it.  fp64: log of the rounded sum, what Ceres computes.  fp32: 1 + x rounds
// x away below 6e-8 and v_log_f32 has only absolute accuracy near 1 -- residuals under ~1e-3 would contribute nothing
// (or noise) to the cost, and the solve would stop on "cost = 0" short of the fp64 pose (scripts/soak.py found a
// zero-residual problem ending 1.1e-4 rad away).  Below 2^-7 the series x (1 - x/2 + x^2/3) is used instead: relative
// error < 2e-7 there, and the hardware log2 is relatively accurate above.
template <typename T> __device__ __forceinline__ T t_log1p_of(T x, T sum);
template <> __device__ __forceinline__ double t_log1p_of<double>(double, double sum) { return t_log<double>(sum); }
template <> __device__ __forceinline__ float t_log1p_of<float>(float x, float sum) {
  const float series = x * __builtin_fmaf(x, __builtin_fmaf(x, 0.33333334f, -0.5f), 1.0f);
  return x < 0.0078125f ? series : t_log<float>(sum);
}

template <typename T>
__device__ __forceinline__ void loss_eval(int kind, T a, T inv_b, T s, T &rho, T &w) {
  if (kind == 1) {  // Cauchy
    const T b = a * a;
    const T x = s * inv_b;
    const T sum = x + T(1);
    w = t_rcp<T>(sum);
    rho = b * t_log1p_of<T>(x, sum);
  } else if (kind == 2) {  // Huber
    const T b = a * a;
    if (s > b) {
      const T r = t_sqrt<T>(s);
      rho = t_fma<T>(T(2) * a, r, -b);
      w = a * t_rcp<T>(r);
    } else {
      rho = s; w = T(1);
    }
  } else {
    rho = s; w = T(1);
  }
}

// The loss of one point and its share of the lane's cost: what fused_chunk and cost_item do behind the sample, in two steps
// because fused_chunk's products sit between them.  loss_point: rho and the IRLS weight w, both 0 for a lane without a valid
// point; `wt` is the point's weight of a weighted term (VAR; ceres::ScaledLoss: a rho, a rho').  cost_point: point k of PPT
// into `cost`.
//
// fp64 lanes with two points under an unweighted Cauchy loss (`pair`, wave-uniform) take ONE logarithm for both: the cost
// only needs log(s0) + log(s1) (pl_log_pair, ea_pair_log.h).  There loss_point returns s = 1 + r^2 / a^2 in place of rho --
// exactly 1 for a lane without a valid point (log 1 = 0: the select that zeroed rho, moved to s) -- point 0 leaves it in
// `held` and point 1 sets the cost to (a^2 / 2) log(s0 s1).  w = 1 / s stays per point: JtJ and Jtr keep their bits, the
// cost moves in its last places.  Everything else -- one point per lane, fp32, weighted terms, Huber, trivial -- is the
// text it was.
template <typename T, int PPT> constexpr bool kPairLog = sizeof(T) == 8 && PPT == 2;
template <typename T, int PPT, bool VAR>
__device__ __forceinline__ void loss_point(bool pair, int kind, T a, T inv_b, T s, bool valid, T wt, T &rho, T &w) {
  if constexpr (kPairLog<T, PPT>) {
    if (pair) {
      const T x = s * inv_b;  // (loss_eval's Cauchy branch, the same expressions)
      const T sum = x + T(1);
      w = t_rcp<T>(sum);
      w = valid ? w : T(0);
      rho = valid ? sum : T(1);
      return;
    }
  }
  loss_eval<T>(kind, a, inv_b, s, rho, w);
  if constexpr (VAR) { w *= wt; rho *= wt; }
  w = valid ? w : T(0);
  rho = valid ? rho : T(0);
}
template <typename T, int PPT>
__device__ __forceinline__ void cost_point(int k, bool pair, T a, T rho, T &cost, T &held) {
  if constexpr (kPairLog<T, PPT>) {
    if (pair) {
      if (k == 0) held = rho;
      else cost = (T(0.5) * (a * a)) * pl_log_pair<LogOps>(held, rho);
      return;
    }
  }
  cost = k == 0 ? T(0.5) * rho : t_fma<T>(T(0.5), rho, cost);
}

// raw 1x6 row of one point from its sample gradient
template <typename T, typename PS>
__device__ __forceinline__ void jacobian_row(const ProblemDesc &pd, const PS &ps,
                                             const Proj<T> &pr, T x, T y, T z, T Fu, T Fv, T J[6]) {
  const T gx = Fu * pr.fxz;
  const T gy = Fv * pr.fyz;
  const T gz = -t_fma<T>(gx, pr.bx, gy * pr.by) * pr.iz;
  if (PoseAcc<T>::unit_q(ps)) {
    // d b / d delta = -2 [R a]x  =>  J_delta = 2 (R a) x g
    J[0] = T(2) * t_fma<T>(pr.cy_, gz, -(pr.cz_ * gy));
    J[1] = T(2) * t_fma<T>(pr.cz_, gx, -(pr.cx_ * gz));
    J[2] = T(2) * t_fma<T>(pr.cx_, gy, -(pr.cy_ * gx));
  } else {
    // (the empty asm keeps this uniform branch a branch: left alone, the compiler computes the 30 extra FMAs of the
    // general path for every point and selects afterwards)
    asm volatile("" ::: "memory");
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const T *G = PoseAcc<T>::G(ps) + 9 * j;
      const T d0 = t_fma<T>(G[2], z, t_fma<T>(G[1], y, G[0] * x));
      const T d1 = t_fma<T>(G[5], z, t_fma<T>(G[4], y, G[3] * x));
      const T d2 = t_fma<T>(G[8], z, t_fma<T>(G[7], y, G[6] * x));
      J[j] = t_fma<T>(gz, d2, t_fma<T>(gy, d1, gx * d0));
    }
  }
  J[3] = gx; J[4] = gy; J[5] = gz;
}

// ------------------------------------------------------------------------------------------------
// wavefront reduction of 32 values per lane: a transposing butterfly.
//
// Each step pairs lanes, lets the pair split its values in two halves, and adds the partner's
// copy of the kept half -- so the number of live values halves while the number of lanes summed
// doubles: 16+8+4+2+1 exchanges instead of 32*6.  The pairings are the ones the hardware offers
// cheaply: lane-swap instructions across half-waves and 16-lane rows (L ^ 32, L ^ 16), DPP inside a
// row (row_mirror = xor 15, row_half_mirror = xor 7, quad_perm = xor 2 and xor 1).  The fp32 and the
// fp64 forms below differ in the order of the levels and hence in the slot a lane ends up with.

constexpr int kDppRowMirror = 0x140, kDppRowHalfMirror = 0x141, kDppQuadXor2 = 0x4E, kDppQuadXor1 = 0xB1;

template <int CTRL>
__device__ __forceinline__ float lane_xchg(float x) {
  // (bound_ctrl: every lane of these patterns has a source lane, so no "old" value is needed -- and none is materialised)
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xF, 0xF, true));
}
template <int CTRL>
__device__ __forceinline__ double lane_xchg(double x) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, x);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)u, CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(u >> 32), CTRL, 0xF, 0xF, true);
  return __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ int wave_min_i32(int x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x = min(x, __shfl_xor(x, m, 64));
  return x;
}
__device__ __forceinline__ int wave_max_i32(int x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x = max(x, __shfl_xor(x, m, 64));
  return x;
}

// ------------------------------------------------------------------------------------------------
// fp32 wavefront reduction with write-masked DPP adds and lane-swap instructions (gfx950).
//
// Same transposing idea as wave_reduce32, but the "keep my half, add the partner's copy" step is
// two instructions and no select:
//   t = lo + dpp(lo)                       all lanes
//   t = hi + dpp(hi)   bank_mask / rows    only the lanes that keep the upper half
// row_mirror pairs lane L with L^15 and the banks 2,3 (L&8) take the upper half; row_half_mirror
// pairs L with L^7, banks 1,3 (L&4).  The cross-row steps use v_permlane16_swap / v_permlane32_swap:
// swapping the odd rows (upper half-wave) of `lo` with the even rows (lower half-wave) of `hi` and
// adding the two results is exactly the transposing step for L^16 (L^32).  Two plain quad_perm
// adds finish the four lanes of a quad.  64 VALU instructions for 32 slots.
// On return lanes with (L & 3) == 0 hold slots  j + 2*b5 + 4*b4 + 8*b2 + 16*b3  in v[j], j = 0, 1.
//
// The DPP adds are inline asm: hipcc cannot see their read-after-write wait states, so every block
// starts with `s_nop 1` (VALU write -> DPP read of the same VGPR needs two wait states).

#define EA_DPP_FULL(o, a, CTRL) "v_add_f32_dpp %" #o ", %" #a ", %" #a " " CTRL " row_mask:0xf bank_mask:0xf\n\t"
#define EA_DPP_MASK(o, a, CTRL, BM) "v_add_f32_dpp %" #o ", %" #a ", %" #a " " CTRL " row_mask:0xf bank_mask:" BM "\n\t"
#define EA_DPP_LEVEL8(CTRL, BM)                                                                              \
  "s_nop 1\n\t" EA_DPP_FULL(0, 8, CTRL) EA_DPP_FULL(1, 9, CTRL) EA_DPP_FULL(2, 10, CTRL) EA_DPP_FULL(3, 11, CTRL) \
      EA_DPP_FULL(4, 12, CTRL) EA_DPP_FULL(5, 13, CTRL) EA_DPP_FULL(6, 14, CTRL) EA_DPP_FULL(7, 15, CTRL)         \
          EA_DPP_MASK(0, 16, CTRL, BM) EA_DPP_MASK(1, 17, CTRL, BM) EA_DPP_MASK(2, 18, CTRL, BM)                 \
              EA_DPP_MASK(3, 19, CTRL, BM) EA_DPP_MASK(4, 20, CTRL, BM) EA_DPP_MASK(5, 21, CTRL, BM)             \
                  EA_DPP_MASK(6, 22, CTRL, BM) EA_DPP_MASK(7, 23, CTRL, BM)

// o[i] = (lanes selected by BM ? hi[i] + partner(hi[i]) : lo[i] + partner(lo[i])), 8 pairs
#define EA_DPP_CALL8(CTRL, BM, o, lo, hi)                                                                     \
  asm volatile(EA_DPP_LEVEL8(CTRL, BM)                                                                         \
               : "=&v"(o[0]), "=&v"(o[1]), "=&v"(o[2]), "=&v"(o[3]), "=&v"(o[4]), "=&v"(o[5]), "=&v"(o[6]), "=&v"(o[7]) \
               : "v"(lo[0]), "v"(lo[1]), "v"(lo[2]), "v"(lo[3]), "v"(lo[4]), "v"(lo[5]), "v"(lo[6]), "v"(lo[7]),  \
                 "v"(hi[0]), "v"(hi[1]), "v"(hi[2]), "v"(hi[3]), "v"(hi[4]), "v"(hi[5]), "v"(hi[6]), "v"(hi[7]))

// v_permlane16_swap / v_permlane32_swap through inline asm (with ROCm 7.2's hipcc the second result of
// __builtin_amdgcn_permlane*_swap aliases the first).  Both operands are swapped in place; the
// leading s_nop covers the VALU-write -> permlane-swap-read wait states hipcc cannot see inside asm.
__device__ __forceinline__ void swap16_x4(float (&lo)[4], float (&hi)[4]) {
  asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %4\n\tv_permlane16_swap_b32 %1, %5\n\t"
               "v_permlane16_swap_b32 %2, %6\n\tv_permlane16_swap_b32 %3, %7\n\ts_nop 0"
               : "+v"(lo[0]), "+v"(lo[1]), "+v"(lo[2]), "+v"(lo[3]), "+v"(hi[0]), "+v"(hi[1]), "+v"(hi[2]), "+v"(hi[3]));
}
__device__ __forceinline__ void swap32_x2(float (&lo)[2], float (&hi)[2]) {
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %2\n\tv_permlane32_swap_b32 %1, %3\n\ts_nop 0"
               : "+v"(lo[0]), "+v"(lo[1]), "+v"(hi[0]), "+v"(hi[1]));
}

// levels C and D of the fp32 reduction: 8 values -> 2 (see wave_reduce32_f32)
__device__ __forceinline__ void swap_levels(const float (&b)[8], float (&c)[4], float (&d)[2]) {
  float lo4[4] = {b[0], b[1], b[2], b[3]}, hi4[4] = {b[4], b[5], b[6], b[7]};
  swap16_x4(lo4, hi4);
#pragma unroll
  for (int i = 0; i < 4; ++i) c[i] = lo4[i] + hi4[i];
  float lo2[2] = {c[0], c[1]}, hi2[2] = {c[2], c[3]};
  swap32_x2(lo2, hi2);
#pragma unroll
  for (int i = 0; i < 2; ++i) d[i] = lo2[i] + hi2[i];
}

__device__ __forceinline__ int masked_slot(int lane, int j) {
  return j + ((lane & 32) >> 4) + ((lane & 16) >> 2) + ((lane & 4) << 1) + ((lane & 8) << 1);
}

__device__ __forceinline__ void wave_reduce32_f32(float (&v)[32]) {
  float a[16], b[8];
  {
    float *o = a, *lo = v, *hi = v + 16;
    EA_DPP_CALL8("row_mirror", "0xc", o, lo, hi);
  }
  {
    float *o = a + 8, *lo = v + 8, *hi = v + 24;
    EA_DPP_CALL8("row_mirror", "0xc", o, lo, hi);
  }
  {
    float *o = b, *lo = a, *hi = a + 8;
    EA_DPP_CALL8("row_half_mirror", "0xa", o, lo, hi);
  }
  float c[4], d[2];
  swap_levels(b, c, d);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    d[i] += lane_xchg<kDppQuadXor1>(d[i]);
    d[i] += lane_xchg<kDppQuadXor2>(d[i]);
  }
  v[0] = d[0];
  v[1] = d[1];
}

// fp64 wavefront reduction with lane-swap instructions for the two widest levels.
//
// v_permlane32_swap exchanges lanes 32..63 of one register with lanes 0..31 of another: applied to slot i and slot
// i + 16 (both dwords of the double), the sum of the two registers is exactly the transposing step for the pairing
// L ^ 32 -- lower half-wave keeps slot i, upper half-wave slot i + 16 -- in three instructions per pair of slots and
// with no select (the DPP form costs seven).  v_permlane16_swap does the same between odd and even 16-lane rows
// (pairing L ^ 16).  The three levels inside a row stay on DPP (row_mirror, row_half_mirror, quad_perm), the last
// pairing (L ^ 1) is a plain add.  ~125 instructions instead of ~220.
// On return lanes with even L hold in v[0] the wave total of slot  16 b5 + 8 b4 + 4 b3 + 2 b2 + b1  (b_k = bit k of L).
// four pairs of doubles per asm statement: one pair of wait-state s_nops (VALU write -> permlane-swap read, swap
// write -> VALU read; hipcc cannot see inside the asm) per eight swaps instead of per two
#define EA_SWAP8(OP)                                                                                        \
  "s_nop 1\n\t" OP " %0, %8\n\t" OP " %1, %9\n\t" OP " %2, %10\n\t" OP " %3, %11\n\t" OP " %4, %12\n\t" \
  OP " %5, %13\n\t" OP " %6, %14\n\t" OP " %7, %15\n\ts_nop 0"
template <int W>  // W = 32: v_permlane32_swap, 16: v_permlane16_swap; a[k] <-> b[k] for k = 0..3 (both dwords)
__device__ __forceinline__ void swap_f64x4(double *a, double *b) {
  unsigned al[4], ah[4], bl[4], bh[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned long long ua = __builtin_bit_cast(unsigned long long, a[k]), ub = __builtin_bit_cast(unsigned long long, b[k]);
    al[k] = (unsigned)ua; ah[k] = (unsigned)(ua >> 32); bl[k] = (unsigned)ub; bh[k] = (unsigned)(ub >> 32);
  }
  if constexpr (W == 32)
    asm volatile(EA_SWAP8("v_permlane32_swap_b32")
                 : "+v"(al[0]), "+v"(ah[0]), "+v"(al[1]), "+v"(ah[1]), "+v"(al[2]), "+v"(ah[2]), "+v"(al[3]), "+v"(ah[3]),
                   "+v"(bl[0]), "+v"(bh[0]), "+v"(bl[1]), "+v"(bh[1]), "+v"(bl[2]), "+v"(bh[2]), "+v"(bl[3]), "+v"(bh[3]));
  else
    asm volatile(EA_SWAP8("v_permlane16_swap_b32")
                 : "+v"(al[0]), "+v"(ah[0]), "+v"(al[1]), "+v"(ah[1]), "+v"(al[2]), "+v"(ah[2]), "+v"(al[3]), "+v"(ah[3]),
                   "+v"(bl[0]), "+v"(bh[0]), "+v"(bl[1]), "+v"(bh[1]), "+v"(bl[2]), "+v"(bh[2]), "+v"(bl[3]), "+v"(bh[3]));
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    a[k] = __builtin_bit_cast(double, ((unsigned long long)ah[k] << 32) | al[k]);
    b[k] = __builtin_bit_cast(double, ((unsigned long long)bh[k] << 32) | bl[k]);
  }
}

__device__ __forceinline__ int swap_slot_f64(int lane) {
  return ((lane & 32) >> 1) | ((lane & 16) >> 1) | ((lane & 8) >> 1) | ((lane & 4) >> 1) | ((lane & 2) >> 1);
}

__device__ __forceinline__ void wave_reduce32_f64(double (&v)[32], int lane) {
#pragma unroll
  for (int i = 0; i < 16; i += 4) {  // L ^ 32
    swap_f64x4<32>(v + i, v + i + 16);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[i + k] += v[i + k + 16];
  }
#pragma unroll
  for (int i = 0; i < 8; i += 4) {  // L ^ 16
    swap_f64x4<16>(v + i, v + i + 8);
#pragma unroll
    for (int k = 0; k < 4; ++k) v[i + k] += v[i + k + 8];
  }
  // inside a 16-lane row: L ^ 15 (bit 3 picks the half kept), L ^ 7 (bit 2), L ^ 2 (bit 1)
  {
    const bool upper = (lane & 8) != 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const double send = upper ? v[i] : v[i + 4];
      const double keep = upper ? v[i + 4] : v[i];
      v[i] = keep + lane_xchg<kDppRowMirror>(send);
    }
  }
  {
    const bool upper = (lane & 4) != 0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const double send = upper ? v[i] : v[i + 2];
      const double keep = upper ? v[i + 2] : v[i];
      v[i] = keep + lane_xchg<kDppRowHalfMirror>(send);
    }
  }
  {
    const bool upper = (lane & 2) != 0;
    const double send = upper ? v[0] : v[1];
    const double keep = upper ? v[1] : v[0];
    v[0] = keep + lane_xchg<kDppQuadXor2>(send);
  }
  v[0] += lane_xchg<kDppQuadXor1>(v[0]);
}

#ifndef EA_TU_VARIANT
// self-test of the cross-lane primitives: one wave, lane L loads in[s*64+L] for slot s; dumps the
// stages of wave_reduce32_f32 (a: 16x64, b: 8x64, c: 4x64, d: 2x64) and the fp64 butterfly result
__global__ void ea_selftest_reduce_kernel(const float *in, float *stage_a, float *stage_b, float *stage_c,
                                          float *stage_d, double *out_f32 /*32*/, double *out_f64 /*32*/) {
  const int lane = threadIdx.x & 63;
  float v[32];
#pragma unroll
  for (int s = 0; s < 32; ++s) v[s] = in[s * 64 + lane];
  double w[32];
#pragma unroll
  for (int s = 0; s < 32; ++s) w[s] = (double)v[s];
  float a[16], b[8];
  { float *o = a, *lo = v, *hi = v + 16; EA_DPP_CALL8("row_mirror", "0xc", o, lo, hi); }
  { float *o = a + 8, *lo = v + 8, *hi = v + 24; EA_DPP_CALL8("row_mirror", "0xc", o, lo, hi); }
  { float *o = b, *lo = a, *hi = a + 8; EA_DPP_CALL8("row_half_mirror", "0xa", o, lo, hi); }
  float c[4], d[2];
  swap_levels(b, c, d);
#pragma unroll
  for (int i = 0; i < 16; ++i) stage_a[i * 64 + lane] = a[i];
#pragma unroll
  for (int i = 0; i < 8; ++i) stage_b[i * 64 + lane] = b[i];
#pragma unroll
  for (int i = 0; i < 4; ++i) stage_c[i * 64 + lane] = c[i];
#pragma unroll
  for (int i = 0; i < 2; ++i) stage_d[i * 64 + lane] = d[i];
  wave_reduce32_f32(v);
  if ((lane & 3) == 0) {
    out_f32[masked_slot(lane, 0)] = (double)v[0];
    out_f32[masked_slot(lane, 1)] = (double)v[1];
  }
  wave_reduce32_f64(w, lane);
  if ((lane & 1) == 0) out_f64[swap_slot_f64(lane)] = w[0];
}
#endif  // !EA_TU_VARIANT

template <typename T> using GPtr = const T __attribute__((address_space(1))) *;

// four consecutive texels through a global-address-space pointer (merged into dwordx4 loads)
template <typename T>
__device__ __forceinline__ Row4<T> load_row4(GPtr<T> p) {
  Row4<T> r;
  r.p0 = p[0]; r.p1 = p[1]; r.p2 = p[2]; r.p3 = p[3];
  return r;
}

// ------------------------------------------------------------------------------------------------
// raw-buffer addressing (gfx950 buffer instructions): a lane's address is ONE 32-bit byte offset and the four
// stencil rows of a point differ only in the instruction's SGPR offset (l * pitch bytes) -- no 64-bit address
// arithmetic per row (ten v_lshl_add_u64 per point in the flat-address form).  Requires the padded image to be
// smaller than 2 GiB (checked on the host, which falls back to the flat-address kernels otherwise).

typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef double f64x2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_raw_buffer(const void *base, unsigned bytes) {
  // gfx950 raw buffer: stride 0, no swizzle, DATA_FORMAT = 32 (dword 3 = 0x00020000)
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, (int)bytes, 0x00020000);
}

template <typename T> __device__ __forceinline__ T buf_load_elem(__amdgpu_buffer_rsrc_t r, int voff);
template <> __device__ __forceinline__ float buf_load_elem<float>(__amdgpu_buffer_rsrc_t r, int voff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, 0, 0));
}
template <> __device__ __forceinline__ double buf_load_elem<double>(__amdgpu_buffer_rsrc_t r, int voff) {
  return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, voff, 0, 0));
}

template <typename T> __device__ __forceinline__ Row4<T> buf_load_row4(__amdgpu_buffer_rsrc_t r, int voff, int soff);
template <> __device__ __forceinline__ Row4<float> buf_load_row4<float>(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
  // (whole-vector bit casts: __builtin_bit_cast of a single element of the loaded vector, `v.x`, comes out of
  // ROCm 7.2's hipcc as four reads of the same dword)
  const f32x4_t v = __builtin_bit_cast(f32x4_t, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
  Row4<float> o;
  o.p0 = v[0]; o.p1 = v[1]; o.p2 = v[2]; o.p3 = v[3];
  return o;
}
template <> __device__ __forceinline__ Row4<double> buf_load_row4<double>(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
  const f64x2_t a = __builtin_bit_cast(f64x2_t, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
  const f64x2_t b = __builtin_bit_cast(f64x2_t, __builtin_amdgcn_raw_buffer_load_b128(r, voff + 16, soff, 0));
  Row4<double> o;
  o.p0 = a[0]; o.p1 = a[1]; o.p2 = b[0]; o.p3 = b[1];
  return o;
}

// A stencil row of a T-typed kernel out of an image stored as IT (IT = T, or float under a double kernel: the fp32-stored
// distance transform of an fp64 problem -- ONE 16-byte load per row and four exact conversions instead of two loads).
template <typename T, typename IT> struct RowLoad {
  static __device__ __forceinline__ Row4<T> buf(__amdgpu_buffer_rsrc_t r, int voff, int soff) { return buf_load_row4<T>(r, voff, soff); }
  static __device__ __forceinline__ Row4<T> flat(GPtr<IT> p) { return load_row4<T>(p); }
};
template <> struct RowLoad<double, float> {
  static __device__ __forceinline__ Row4<double> buf(__amdgpu_buffer_rsrc_t r, int voff, int soff) {
    const Row4<float> f = buf_load_row4<float>(r, voff, soff);
    Row4<double> o;
    o.p0 = (double)f.p0; o.p1 = (double)f.p1; o.p2 = (double)f.p2; o.p3 = (double)f.p3;
    return o;
  }
  static __device__ __forceinline__ Row4<double> flat(GPtr<float> p) {
    const Row4<float> f = load_row4<float>(p);
    Row4<double> o;
    o.p0 = (double)f.p0; o.p1 = (double)f.p1; o.p2 = (double)f.p2; o.p3 = (double)f.p3;
    return o;
  }
};
template <typename T, bool IMG32> struct ImgOf { typedef T type; };
template <> struct ImgOf<double, true> { typedef float type; };

// ------------------------------------------------------------------------------------------------
// The wave-exchange reduction of a 256-lane fp64 workgroup (ea_wave_exchange.h has the ownership arithmetic and the LDS
// layout): the four wavefronts add their 32 sums lane by lane through LDS in two halving rounds, so that each runs the
// butterfly over the 8 slots it ends up owning instead of over all 32 -- 12 lane swaps per wavefront instead of 48, the
// work spread evenly over the four SIMDs.  Which half a wavefront keeps is wave-uniform: branches, no per-lane selects.
// Returns the finished sum of slot xchg_store_slot(wave, lane) in the lanes that have one.
#define EA_SWAP4(OP) "s_nop 1\n\t" OP " %0, %4\n\t" OP " %1, %5\n\t" OP " %2, %6\n\t" OP " %3, %7\n\ts_nop 0"
// the two-double twin of swap_f64x4<16>: a[k] <-> b[k] for k = 0, 1 between odd and even 16-lane rows
__device__ __forceinline__ void swap16_f64x2(double *a, double *b) {
  unsigned al[2], ah[2], bl[2], bh[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const unsigned long long ua = __builtin_bit_cast(unsigned long long, a[k]), ub = __builtin_bit_cast(unsigned long long, b[k]);
    al[k] = (unsigned)ua; ah[k] = (unsigned)(ua >> 32); bl[k] = (unsigned)ub; bh[k] = (unsigned)(ub >> 32);
  }
  asm volatile(EA_SWAP4("v_permlane16_swap_b32")
               : "+v"(al[0]), "+v"(ah[0]), "+v"(al[1]), "+v"(ah[1]), "+v"(bl[0]), "+v"(bh[0]), "+v"(bl[1]), "+v"(bh[1]));
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    a[k] = __builtin_bit_cast(double, ((unsigned long long)ah[k] << 32) | al[k]);
    b[k] = __builtin_bit_cast(double, ((unsigned long long)bh[k] << 32) | bl[k]);
  }
}

// (The two halves of a uniform branch differ only in which registers they name, which invites the compiler to merge them
// into one copy behind per-lane selects -- 64 v_cndmask_b32 -- or to join them through register copies.  An empty asm
// statement of its own at either end of each half keeps the halves apart: nothing is hoisted, sunk or if-converted across it.)
#define EA_XCHG_HALF(TAG, ...) do { asm volatile("; " TAG); __VA_ARGS__ asm volatile("; " TAG " end"); } while (0)
// (... and the sums of a half, which have no side effect to hold them there, leave it through an asm statement's operands)
#define EA_XCHG_PIN8(TAG, X) asm volatile("; " TAG : "+v"((X)[0]), "+v"((X)[1]), "+v"((X)[2]), "+v"((X)[3]), "+v"((X)[4]), "+v"((X)[5]), "+v"((X)[6]), "+v"((X)[7]))
__device__ __forceinline__ double wave_exchange_reduce_f64(const double (&v)[32], int wave, int lane, unsigned char *lds /* kXchgBytes */) {
  const int w = __builtin_amdgcn_readfirstlane(wave);
  auto cells = [&](int region) { return reinterpret_cast<f64x2_t *>(lds + xchg_cell_offset(region, 0, lane)); };
  constexpr int kPair = 1024 / (int)sizeof(f64x2_t);  // cells 2p, 2p + 1 of a lane: p * kPair vectors on
  const bool hi16 = xchg_keep16(w) != 0, hi8 = xchg_keep8(w) != 0;  // (wave-uniform)
  // round 1: w <-> w ^ 1, 16 of 32
  double k[16];
  {
    f64x2_t *out = cells(xchg_write_region1(w));
    auto store = [&](const double *from) {
#pragma unroll
      for (int p = 0; p < 8; ++p) { f64x2_t o; o[0] = from[2 * p]; o[1] = from[2 * p + 1]; out[p * kPair] = o; }
    };
    if (hi16) EA_XCHG_HALF("exchange 1: keep 16..31", store(v););
    else EA_XCHG_HALF("exchange 1: keep 0..15", store(v + 16););
    __syncthreads();
    const f64x2_t *in = cells(xchg_read_region1(w));
    f64x2_t a[8];
#pragma unroll
    for (int p = 0; p < 8; ++p) a[p] = in[p * kPair];
    auto sum = [&](const double *kept) {
#pragma unroll
      for (int p = 0; p < 8; ++p) { k[2 * p] = kept[2 * p] + a[p][0]; k[2 * p + 1] = kept[2 * p + 1] + a[p][1]; }
    };
    if (hi16) EA_XCHG_HALF("exchange 1: sum 16..31", sum(v + 16); EA_XCHG_PIN8("16..23", k); EA_XCHG_PIN8("24..31", k + 8););
    else EA_XCHG_HALF("exchange 1: sum 0..15", sum(v); EA_XCHG_PIN8("0..7", k); EA_XCHG_PIN8("8..15", k + 8););
  }
  // round 2: w <-> w ^ 2, 8 of 16, into the region this wavefront has just read
  double e[8];
  {
    f64x2_t *out = cells(xchg_write_region2(w));
    auto store = [&](const double *from) {
#pragma unroll
      for (int p = 0; p < 4; ++p) { f64x2_t o; o[0] = from[2 * p]; o[1] = from[2 * p + 1]; out[p * kPair] = o; }
    };
    if (hi8) EA_XCHG_HALF("exchange 2: keep 8..15", store(k););
    else EA_XCHG_HALF("exchange 2: keep 0..7", store(k + 8););
    __syncthreads();
    const f64x2_t *in = cells(xchg_read_region2(w));
    f64x2_t a[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) a[p] = in[p * kPair];
    auto sum = [&](const double *kept) {
#pragma unroll
      for (int p = 0; p < 4; ++p) { e[2 * p] = kept[2 * p] + a[p][0]; e[2 * p + 1] = kept[2 * p + 1] + a[p][1]; }
    };
    if (hi8) EA_XCHG_HALF("exchange 2: sum 8..15", sum(k + 8); EA_XCHG_PIN8("8..15", e););
    else EA_XCHG_HALF("exchange 2: sum 0..7", sum(k); EA_XCHG_PIN8("0..7", e););
  }
  // the butterfly over the 8 values this wavefront owns: L ^ 32, L ^ 16, L ^ 15 halve, L ^ 7, L ^ 2, L ^ 1 add the partner
  swap_f64x4<32>(e, e + 4);
#pragma unroll
  for (int i = 0; i < 4; ++i) e[i] += e[i + 4];
  swap16_f64x2(e, e + 2);
#pragma unroll
  for (int i = 0; i < 2; ++i) e[i] += e[i + 2];
  const bool upper = (lane & 8) != 0;
  const double send = upper ? e[0] : e[1];
  const double keep = upper ? e[1] : e[0];
  double r = keep + lane_xchg<kDppRowMirror>(send);
  r += lane_xchg<kDppRowHalfMirror>(r);
  r += lane_xchg<kDppQuadXor2>(r);
  r += lane_xchg<kDppQuadXor1>(r);
  return r;
}

// ------------------------------------------------------------------------------------------------
// fused evaluation kernel: residual + Jacobian + loss + JtJ/Jtr/cost partials, one row per workgroup
//
// grid = (8 * ceil(chunks/8), problems).  Workgroup (c, p) owns points [c*chunk, (c+1)*chunk) of
// problem p, chunk = NT*PPT: every lane takes PPT points (strided by NT so loads coalesce), one
// wavefront butterfly per wave and one cross-wave fold per workgroup -> one partial row.

// the weight of stored point i of a weighted term (ProblemDesc::w_off), NULL for a term without weights
template <typename T> __device__ __forceinline__ const T *desc_weights(const ProblemDesc &pd, long long i) {
  return (pd.variant & 4) ? static_cast<const T *>(pd.z) + pd.w_off + i : nullptr;
}

constexpr int kMaxWaves = 16;
// MODE of ea_eval_poses_kernel / ea_eval_starts_kernel only: MODE 0's per-point code with the wave-exchange reduction (fp64, 256
// lanes); the dynamic LDS of such a launch is the exchange buffer (kXchgBytes)
constexpr int kModeExchange = 3;
constexpr int kRedBytes = kMaxWaves * kAccSlots * 8;  // cross-wave scratch: up to 16 waves x 32 doubles
constexpr int kHdrBytes = kRedBytes + kMaxWaves * 16;  // + bbox words, keeps the tile 16-byte aligned

// One workgroup's share of an evaluation: NT lanes x PPT points -> the workgroup's partial row.
// X/Y/Z hold the lane's points (lanes past `count` carry a copy of the chunk's last point); the return value is
// slot `my_slot` of the row (0 when my_slot < 0).  `ps` may live in global memory (scalar loads) or LDS.
// XCHG (fp64, 256 lanes, MODE 0): the wave-exchange reduction above instead of a 32-value butterfly per wavefront and the
// cross-wave sum; s_red is then the kXchgBytes exchange buffer, my_slot is not read, and the return value is the sum of slot
// xchg_store_slot(wave, lane) in the lanes that have one (another fixed summation order: the last place may differ).
template <typename T, int PPT, int MODE, int NT, bool VAR, bool BUF, bool IMG32, typename PS, bool XCHG = false>
__device__ __forceinline__ double fused_chunk(const ProblemDesc &pd, const PS &ps, const T (&X)[PPT],
                                              const T (&Y)[PPT], const T (&Z)[PPT], int count, double *s_red,
                                              int *s_box, T *s_tile, int lds_texels, int my_slot,
                                              const T *wts = nullptr) {
  // MODE 0: stencil rows from L2.  1: DT footprint staged in LDS.  2: as 0, and an fp32 kernel widens a lane's sums to
  // fp64 before the wavefront butterfly ("wide_accumulate": everything above a lane's <= PPT products is fp64).
  constexpr bool USE_LDS = MODE == 1;
  constexpr bool WIDE = MODE == 2 && sizeof(T) == 4;
  static_assert(!IMG32 || (std::is_same<T, double>::value && MODE == 0 && !VAR), "fp32-stored image: plain fp64 kernels on the L2 path");
  static_assert(!XCHG || (sizeof(T) == 8 && NT == 256 && MODE == 0), "wave exchange: fp64, four wavefronts, L2 path");
  typedef typename ImgOf<T, IMG32>::type IT;  // element type of the image in HBM
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int pitch = pd.pitch;
  const void *img_base = IMG32 ? pd.dt32 : pd.dt;
  const GPtr<IT> gimg = (GPtr<IT>)(static_cast<const IT *>(img_base) + (size_t)kImagePad * (size_t)pitch + kImagePad);
  const __amdgpu_buffer_rsrc_t rimg =
      make_raw_buffer(img_base, BUF ? (unsigned)pitch * (unsigned)(pd.H + 2 * kImagePad) * (unsigned)sizeof(IT) : 0u);
  const int loss_kind = pd.loss_kind;
  const T loss_a = Uni<T>::loss_a(pd), loss_inv_b = Uni<T>::loss_inv_b(pd);

  T acc[28];
  int n_bad = 0;
  // VAR: the per-point weights of a weighted term (ProblemDesc::variant bit 2; `wts` = the chunk's first weight, NULL for
  // every other term: one wave-uniform branch, nothing loaded behind it), coalesced like the points.  ceres::ScaledLoss(rho, a)
  // is a rho, a rho': the weight multiplies the IRLS pair behind loss_eval; lanes past the end and failed functors get
  // (0, 0) anyway.  Only the weighted kernels (ea_eval_fused_w_kernel ...) hand a pointer in: everywhere else `wts` is the
  // constant NULL and this folds away.
  T WT[PPT];
  if constexpr (VAR) {
#pragma unroll
    for (int k = 0; k < PPT; ++k) WT[k] = T(1);
    if (wts) {
      const GPtr<T> gw = (GPtr<T>)wts;
#pragma unroll
      for (int k = 0; k < PPT; ++k) WT[k] = gw[min(tid + k * NT, count - 1)];
    }
  }
  // ---- phase 1: warp + projection.  Lanes past the end of the chunk and lanes whose functor fails are moved
  // to a harmless sample; both get weight 0 below, so the arithmetic needs no divergent branch.
  using ProjT = typename std::conditional<VAR, ProjV<T>, Proj<T>>::type;
  ProjT pr[PPT];
  bool valid[PPT];
  int bb_u0 = 0x7fffffff, bb_u1 = -0x7fffffff, bb_v0 = 0x7fffffff, bb_v1 = -0x7fffffff;
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    const bool inb = tid + k * NT < count;
    if constexpr (VAR) project_point_var<T>(pd, ps, X[k], Y[k], Z[k], pr[k]);
    else project_point<T>(pd, ps, X[k], Y[k], Z[k], pr[k]);
    valid[k] = inb && pr[k].state == 1;
    n_bad += (inb && pr[k].state == 2) ? 1 : 0;
    if (__any(!valid[k]) && !valid[k]) {  // (uniform test first: the common wavefront has nothing to fix up)
      pr[k].iu = 0; pr[k].iv = 0; pr[k].fu = T(0); pr[k].fv = T(0);
      pr[k].iz = T(1);
      if constexpr (VAR) {
        pr[k].x = T(0); pr[k].y = T(0);
        pr[k].xdx = T(1); pr[k].xdy = T(0); pr[k].ydx = T(0); pr[k].ydy = T(1);
      } else {
        pr[k].bx = T(0); pr[k].by = T(0);
        pr[k].fxz = T(0); pr[k].fyz = T(0);
      }
    }
    if (USE_LDS && valid[k]) {
      bb_u0 = min(bb_u0, pr[k].iu); bb_u1 = max(bb_u1, pr[k].iu);
      bb_v0 = min(bb_v0, pr[k].iv); bb_v1 = max(bb_v1, pr[k].iv);
    }
  }
  // (fp64, two points: left to itself the compiler counts the failed functors at the very end and carries the four lane
  // masks there -- eight scalar registers the kernel does not have: spilled to a VGPR's lanes and read back, 16 lane moves
  // per wavefront.  Through a "v" operand the count is made here and the masks die.)
  if constexpr (kPairLog<T, PPT>) asm volatile("" : "+v"(n_bad));

  // ---- phase 2: footprint of the chunk, staged through LDS when it fits
  bool in_lds = false;
  int u0 = 0, v0 = 0, tw = 0;
  if (USE_LDS) {
    bb_u0 = wave_min_i32(bb_u0); bb_u1 = wave_max_i32(bb_u1);
    bb_v0 = wave_min_i32(bb_v0); bb_v1 = wave_max_i32(bb_v1);
    if (lane == 0) {
      s_box[4 * wave + 0] = bb_u0; s_box[4 * wave + 1] = bb_u1;
      s_box[4 * wave + 2] = bb_v0; s_box[4 * wave + 3] = bb_v1;
    }
    __syncthreads();
    int U0 = s_box[0], U1 = s_box[1], V0 = s_box[2], V1 = s_box[3];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) {
      U0 = min(U0, s_box[4 * w + 0]); U1 = max(U1, s_box[4 * w + 1]);
      V0 = min(V0, s_box[4 * w + 2]); V1 = max(V1, s_box[4 * w + 3]);
    }
    if (U1 >= U0) {
      u0 = min(U0, 0) - 1; v0 = min(V0, 0) - 1;  // weight-0 lanes sample texel (0,0): keep it inside
      U1 = max(U1, 0); V1 = max(V1, 0);
      tw = U1 - (u0 + 1) + 4;
      const int th = V1 - (v0 + 1) + 4;
      const long long area = (long long)tw * (long long)th;
      if (area <= (long long)lds_texels) {
        in_lds = true;
        const GPtr<IT> img = gimg + ((ptrdiff_t)v0 * pitch + u0);
        const float inv_tw = 1.0f / (float)tw;
        for (int idx = tid; idx < (int)area; idx += NT) {
          int row = (int)((float)idx * inv_tw);
          int col = idx - row * tw;
          if (col < 0) { row -= 1; col += tw; }
          if (col >= tw) { row += 1; col -= tw; }
          s_tile[idx] = img[(ptrdiff_t)row * pitch + col];
        }
        __syncthreads();
      }
    }
  }

  EA_STAMP(3);  // projected
  // ---- phase 3: sample, Jacobian, weights, accumulate
  const bool pair = loss_kind == 1 && (!VAR || wts == nullptr);  // one log per lane (loss_point)
  T held = T(1);
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    T f, Fu, Fv;
    if (USE_LDS && in_lds) {
      const T *base = s_tile + (pr[k].iv - 1 - v0) * tw + (pr[k].iu - 1 - u0);
      const int stride = tw;
      bicubic<T>(pr[k].fu, pr[k].fv,
                 [&](int l) { return *reinterpret_cast<const Row4<T> *>(base + l * stride); }, f, Fu, Fv);
    } else if constexpr (BUF) {
      // byte offset of texel (iv - 1, iu - 1) in the padded image; iv, iu >= -2 keeps it non-negative
      const int voff = ((pr[k].iv + (kImagePad - 1)) * pitch + (pr[k].iu + (kImagePad - 1))) * (int)sizeof(IT);
      bicubic<T>(pr[k].fu, pr[k].fv,
                 [&](int l) { return RowLoad<T, IT>::buf(rimg, voff, l * pitch * (int)sizeof(IT)); }, f, Fu, Fv);
    } else {
      const GPtr<IT> base = gimg + ((ptrdiff_t)(pr[k].iv - 1) * pitch + (pr[k].iu - 1));
      bicubic<T>(pr[k].fu, pr[k].fv,
                 [&](int l) { return RowLoad<T, IT>::flat(base + (ptrdiff_t)l * pitch); }, f, Fu, Fv);
    }
    T J[6];
    if constexpr (VAR) jacobian_row_var<T>(pd, ps, pr[k], Fu, Fv, J);
    else jacobian_row<T>(pd, ps, pr[k], X[k], Y[k], Z[k], Fu, Fv, J);
    // (every kernel but the fp64 two-point ones keeps the statements it had, here and at the cost below, not loss_point's
    // copy of them: through the helper the one-point kernels came out with two instructions swapped, and they are compared
    // byte for byte with the build before -- scripts/compare_device_code.py)
    T rho, w;
    if constexpr (kPairLog<T, PPT>) {
      T wt = T(1);
      if constexpr (VAR) wt = WT[k];
      loss_point<T, PPT, VAR>(pair, loss_kind, loss_a, loss_inv_b, f * f, valid[k], wt, rho, w);
    } else {
      loss_eval<T>(loss_kind, loss_a, loss_inv_b, f * f, rho, w);
      if constexpr (VAR) { w *= WT[k]; rho *= WT[k]; }
      w = valid[k] ? w : T(0);
      rho = valid[k] ? rho : T(0);
    }
    const T wr = w * f;
    int s = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      const T wJa = w * J[a];
#pragma unroll
      for (int b = a; b < 6; ++b) { acc[s] = k == 0 ? wJa * J[b] : t_fma<T>(wJa, J[b], acc[s]); ++s; }
      acc[kAccJtr + a] = k == 0 ? J[a] * wr : t_fma<T>(J[a], wr, acc[kAccJtr + a]);
    }
    if constexpr (kPairLog<T, PPT>) cost_point<T, PPT>(k, pair, loss_a, rho, acc[kAccCost], held);
    else acc[kAccCost] = k == 0 ? T(0.5) * rho : t_fma<T>(T(0.5), rho, acc[kAccCost]);
  }

  // ---- phase 4: wavefront reduction in the kernel's arithmetic type (a lane's accumulators and
  // a wavefront's 64-lane sums are T; everything above a wavefront is fp64), then the
  // fixed-order cross-wave sum
  T v[32];
#pragma unroll
  for (int i = 0; i < 28; ++i) v[i] = acc[i];
  v[28] = (T)n_bad; v[29] = T(0); v[30] = T(0); v[31] = T(0);
#ifdef EA_STAMPS
  asm volatile("" ::"v"(v[0]), "v"(v[27]));
#endif
  EA_STAMP(4);  // sampled + accumulated
  if (USE_LDS) __syncthreads();  // tile readers done before the scratch rows are written
  if constexpr (XCHG) {
    return wave_exchange_reduce_f64(v, wave, lane, reinterpret_cast<unsigned char *>(s_red));
  } else if constexpr (WIDE) {
    double w[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) w[i] = (double)v[i];
    wave_reduce32_f64(w, lane);
    if ((lane & 1) == 0) s_red[wave * kAccSlots + swap_slot_f64(lane)] = w[0];
  } else if constexpr (sizeof(T) == 4) {
    wave_reduce32_f32(v);
    if ((lane & 3) == 0) {
      s_red[wave * kAccSlots + masked_slot(lane, 0)] = (double)v[0];
      s_red[wave * kAccSlots + masked_slot(lane, 1)] = (double)v[1];
    }
  } else {
    wave_reduce32_f64(v, lane);
    if ((lane & 1) == 0) s_red[wave * kAccSlots + swap_slot_f64(lane)] = v[0];
  }
  EA_STAMP(5);  // wave reduced
  __syncthreads();
  EA_STAMP(6);  // all waves of the workgroup arrived
  double sum = 0.0;
  if (my_slot >= 0) {
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) sum += s_red[w * kAccSlots + my_slot];
  }
  return sum;
}

// a value every lane of the wavefront holds (read from LDS, say) as a scalar-register operand
template <typename T> __device__ __forceinline__ T uniform_scalar(T v);
template <> __device__ __forceinline__ float uniform_scalar<float>(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}
template <> __device__ __forceinline__ double uniform_scalar<double>(double v) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)u), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(u >> 32));
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// ---- the head of a work item -------------------------------------------------------------------------------------------
// What every evaluation kernel does between knowing its (chunk, term, pose slot) and fused_chunk, written ONCE: the kernels'
// promises of equal bits (a start's rows = the pose-batched rows, the fused iteration = the step pair, the flat launch = the
// grid) and any change to what the common path reads rest on this text.  The ORDER of its statements is the point:
//   1. term 0's points -- arrays and count came with the wave (kernarg preload) -- go out first, so that the coalesced point
//      loads travel while descriptor and pose are fetched: one dependent memory round trip less in the chain descriptor ->
//      points -> stencil rows that bounds a small launch;
//   2. descriptor and pose by value, every uniform the common path reads named in front of the early exit, so that they go
//      out as ONE batch of scalar loads behind one wait.  Left alone the compiler fetches what the exit test needs, then the
//      pose's flag, then the rest: three dependent round trips at the head of every workgroup;
//   3. the early exit, then the point loads of every other term, which had to wait for the descriptor.

// A lane's PPT points of a chunk of `count` points, from the three arrays at the chunk's first point: coalesced, a point's
// X, Y, Z issued together; lanes past the end of the chunk re-read its last point.  BUF: the chunk as three raw buffers, one
// 32-bit offset per lane serves all three loads.
template <typename T, int PPT, int NT, bool BUF>
__device__ __forceinline__ void load_chunk_points(const T *px, const T *py, const T *pz, int count, T (&X)[PPT], T (&Y)[PPT],
                                                  T (&Z)[PPT]) {
  const int tid = threadIdx.x;
  if constexpr (BUF) {
    const __amdgpu_buffer_rsrc_t rx = make_raw_buffer(px, (unsigned)count * (unsigned)sizeof(T));
    const __amdgpu_buffer_rsrc_t ry = make_raw_buffer(py, (unsigned)count * (unsigned)sizeof(T));
    const __amdgpu_buffer_rsrc_t rz = make_raw_buffer(pz, (unsigned)count * (unsigned)sizeof(T));
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      const int poff = min(tid + k * NT, count - 1) * (int)sizeof(T);
      X[k] = buf_load_elem<T>(rx, poff); Y[k] = buf_load_elem<T>(ry, poff); Z[k] = buf_load_elem<T>(rz, poff);
    }
  } else {
    const GPtr<T> gx = (GPtr<T>)px, gy = (GPtr<T>)py, gz = (GPtr<T>)pz;
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      const int jj = min(tid + k * NT, count - 1);
      X[k] = gx[jj]; Y[k] = gy[jj]; Z[k] = gz[jj];
    }
  }
}

// the descriptor words every evaluation reads, as operands of an `asm volatile("" :: ...)` that names them in one place
#define EA_DESC_UNIFORMS(T, IMG32, pd)                                                                                     \
  "s"(pd.x), "s"(pd.y), "s"(pd.z), "s"(IMG32 ? pd.dt32 : pd.dt), "s"(pd.n), "s"(pd.W), "s"(pd.H), "s"(pd.pitch),           \
  "s"(Uni<T>::fx(pd)), "s"(Uni<T>::fy(pd)), "s"(Uni<T>::cx(pd)), "s"(Uni<T>::cy(pd)), "s"(Uni<T>::loss_a(pd)),             \
  "s"(Uni<T>::loss_inv_b(pd)), "s"(Uni<T>::z_guard(pd)), "s"(Uni<T>::z_eps(pd)), "s"(pd.loss_kind)

template <typename T>
__device__ __forceinline__ void load_pose_lite(const PoseState *psp, PoseLite<T> &ps, int &active) {
  const T *R_ = Uni<T>::R(*psp), *t_ = Uni<T>::t(*psp);
#pragma unroll
  for (int i = 0; i < 9; ++i) ps.R[i] = R_[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) ps.t[i] = t_[i];
  ps.unit_q = psp->unit_q;
  ps.full = psp;
  active = psp->active;
}

// Step 2: the pose at `psp` into scalars beside the descriptor `pd` (already assigned by value), both pinned.  GRID: the
// (chunks, terms) grid of eval_fused_body also reads the descriptor's row base and pose group.
template <typename T, bool IMG32, bool GRID>
__device__ __forceinline__ void fetch_item_uniforms(const ProblemDesc &pd, const PoseState *psp, PoseLite<T> &ps, int &active) {
  load_pose_lite<T>(psp, ps, active);
  if constexpr (GRID) asm volatile("" ::EA_DESC_UNIFORMS(T, IMG32, pd), "s"(pd.tile_begin), "s"(pd.variant), "s"(pd.group));
  else asm volatile("" ::EA_DESC_UNIFORMS(T, IMG32, pd), "s"(pd.variant));
  asm volatile("" : "+s"(active), "+s"(ps.unit_q), "+s"(ps.R[0]), "+s"(ps.R[1]), "+s"(ps.R[2]), "+s"(ps.R[3]), "+s"(ps.R[4]),
                    "+s"(ps.R[5]), "+s"(ps.R[6]), "+s"(ps.R[7]), "+s"(ps.R[8]), "+s"(ps.t[0]), "+s"(ps.t[1]), "+s"(ps.t[2]));
}

// Steps 1 to 3 for work item (chunk c_ of chunk_ points, term_, pose slot_), as the text of the kernel that names it: behind it
// `pd` (const), `ps`, `X`, `Y`, `Z`, `count` and `start` are the kernel's locals.  NOTHING is the statement of an item with
// nothing to evaluate (`return`, or what the kernel owes for an empty row first).  The pose is fetched SPECULATIVELY from
// slot_, independent of the descriptor; under GRID_ with regroup_ (terms that share poses) a term whose group is another
// slot fetches again (uniform, rare).  Reads the kernel's T, PPT, NT, BUF, IMG32 and x0, y0, z0, n0, probs, poses.
// A macro and not a function: with the descriptor a const local of the kernel and the exits the kernel's own `return`,
// the compiler emits the code of the heads written out (profiles/item_head_listing.md); handed out of a function -- through
// references, or to the rest of the kernel as a continuation -- the fp64 exchange and the cost kernels merge the early and
// the late point loads through register copies and the variant fp64 kernel grows by a tenth.  For the same reason a kernel's
// `const int tid = threadIdx.x` stays in FRONT of the head.
#define EA_ITEM_HEAD(GRID_, chunk_, c_, term_, slot_, regroup_, NOTHING)                                                   \
  const long long start = (long long)(c_) * (chunk_);                                                                      \
  T X[PPT], Y[PPT], Z[PPT];                                                                                                \
  const bool early = BUF && (term_) == 0 && n0 > 0; /* (uniform) */                                                        \
  if (early) {                                                                                                             \
    if (start >= n0) { NOTHING; }                                                                                          \
    load_chunk_points<T, PPT, NT, true>(static_cast<const T *>(x0) + start, static_cast<const T *>(y0) + start,            \
                                        static_cast<const T *>(z0) + start, min((chunk_), (int)(n0 - start)), X, Y, Z);   \
  }                                                                                                                        \
  const ProblemDesc pd = probs[term_];                                                                                     \
  PoseLite<T> ps;                                                                                                          \
  int active;                                                                                                              \
  fetch_item_uniforms<T, IMG32, GRID_>(pd, poses + (slot_), ps, active);                                                   \
  if (GRID_ && (regroup_) && pd.group != (int)(slot_)) load_pose_lite<T>(poses + pd.group, ps, active);                    \
  if (start >= pd.n || !active) { NOTHING; }                                                                               \
  const int count = min((chunk_), (int)(pd.n - start));                                                                    \
  if (!early)                                                                                                              \
    load_chunk_points<T, PPT, NT, BUF>(static_cast<const T *>(pd.x) + start, static_cast<const T *>(pd.y) + start,         \
                                       static_cast<const T *>(pd.z) + start, count, X, Y, Z)

// a finished row sum into slot (tid, or the exchange's slot) of partial row `out_row`
template <bool XCHG>
__device__ __forceinline__ void store_row_sum(double *__restrict__ partials, int out_row, double sum) {
  const int tid = threadIdx.x;
  if constexpr (XCHG) {  // (one lane per (wavefront, slot) holds the finished sum)
    const int slot = xchg_store_slot(tid >> 6, tid & 63);
    if (slot >= 0) partials[(size_t)out_row * kAccSlots + slot] = sum;
  } else {
    if (tid < kAccSlots) partials[(size_t)out_row * kAccSlots + tid] = sum;
  }
}

// NT = workgroup size (256 or 1024).  1024 = one workgroup per CU: four times fewer partial rows
// to fold afterwards at the same points-per-lane latency.
template <typename T, int PPT, int MODE, int NT, bool VAR, bool BUF, bool IMG32, bool WTD = false>
__device__ __forceinline__ void eval_fused_body(
    const void *__restrict__ x0, const void *__restrict__ y0, const void *__restrict__ z0, int n0,
    int shape, int chunks_per_xcd,
    const ProblemDesc *__restrict__ probs, const PoseState *__restrict__ poses,
    double *__restrict__ partials, int lds_texels) {
  const int chunk = shape & 0xffff, xcd_remap = (shape >> 16) & 1, terms_are_groups = (shape >> 17) & 1;
  extern __shared__ __align__(16) unsigned char smem[];
  double *s_red = reinterpret_cast<double *>(smem);
  int *s_box = reinterpret_cast<int *>(smem + kRedBytes);
  T *s_tile = reinterpret_cast<T *>(smem + kHdrBytes);

  // XCD-aware chunk assignment: workgroups are dealt round-robin over the 8 XCDs, so give each
  // XCD a contiguous run of chunks (neighbouring chunks read neighbouring image rows -> one L2).
  EA_STAMP(0);
  const int bx = blockIdx.x;
  const int c = xcd_remap ? (bx & 7) * chunks_per_xcd + (bx >> 3) : bx;
  const int tid = threadIdx.x;
  EA_ITEM_HEAD(true, chunk, c, blockIdx.y, blockIdx.y, !terms_are_groups, return);
  EA_STAMP(1);  // descriptor + pose.active arrived (the late point loads are out)
#ifdef EA_STAMPS
  asm volatile("" ::"v"(X[0]), "v"(Y[0]), "v"(Z[0]));
#endif
  EA_STAMP(2);  // points arrived
  const T *wts = nullptr;
  if constexpr (VAR && WTD) wts = desc_weights<T>(pd, start);
  const double sum = fused_chunk<T, PPT, MODE, NT, VAR, BUF, IMG32, PoseLite<T>>(pd, ps, X, Y, Z, count, s_red, s_box, s_tile, lds_texels,
                                                           tid < kAccSlots ? tid : -1, wts);
  if (tid < kAccSlots) partials[(size_t)(pd.tile_begin + c) * kAccSlots + tid] = sum;
#ifdef EA_STAMPS
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
  EA_STAMP(7);  // row stored
}

template <typename T, int PPT, int MODE, int NT, bool VAR, bool BUF, bool IMG32 = false>
__global__ __launch_bounds__(NT) void ea_eval_fused_kernel(
    // the first 16 dwords of the argument segment arrive in SGPRs with the wave (kernarg preload): what problem 0's point
    // loads need sits there, so that they can be issued at once, beside the descriptor fetch instead of behind it
    // (14 dwords fit beside the argument pointer: three pointers, the count, the launch shape packed into one word --
    // chunk | xcd_remap << 16 | terms_are_groups << 17 --, chunks per XCD, and the descriptor and pose tables)
    const void *__restrict__ x0, const void *__restrict__ y0, const void *__restrict__ z0, int n0,
    int shape, int chunks_per_xcd,
    const ProblemDesc *__restrict__ probs, const PoseState *__restrict__ poses,
    double *__restrict__ partials, int lds_texels) {
  eval_fused_body<T, PPT, MODE, NT, VAR, BUF, IMG32>(x0, y0, z0, n0, shape, chunks_per_xcd, probs, poses, partials, lds_texels);
}

// The same kernel under a second name, for the pose-batched launches of the batches ea_eval_poses_kernel below does not
// cover (variant functors, LDS staging, wide_accumulate, terms that share a pose): grid y = G poses x terms over a
// descriptor table replicated G times.  rocprofv3 --kernel-trace --stats keeps them apart from the one-pose launches of the
// solves and of ea_batch_eval in the same process.  Body, arguments and instantiations are those of ea_eval_fused_kernel.
template <typename T, int PPT, int MODE, int NT, bool VAR, bool BUF, bool IMG32 = false>
__global__ __launch_bounds__(NT) void ea_eval_poses_grid_kernel(
    const void *__restrict__ x0, const void *__restrict__ y0, const void *__restrict__ z0, int n0,
    int shape, int chunks_per_xcd,
    const ProblemDesc *__restrict__ probs, const PoseState *__restrict__ poses,
    double *__restrict__ partials, int lds_texels) {
  eval_fused_body<T, PPT, MODE, NT, VAR, BUF, IMG32>(x0, y0, z0, n0, shape, chunks_per_xcd, probs, poses, partials, lds_texels);
}

#ifdef EA_TU_VARIANT
// The two kernels above for batches with weighted terms (ProblemDesc::variant bit 2; EvalLaunch::weighted): the same body with
// the weights of such terms loaded and multiplied into the IRLS pair.  Kernels of their own, not a branch in the ones above: a
// batch of distortion / second-camera terms without weights runs the code it always ran (the branch alone cost the fp64
// two-point kernel a wave of occupancy: profiles/LOG.md).
template <typename T, int PPT, int MODE, int NT, bool VAR, bool BUF, bool IMG32 = false>
__global__ __launch_bounds__(NT) void ea_eval_fused_w_kernel(
    const void *__restrict__ x0, const void *__restrict__ y0, const void *__restrict__ z0, int n0,
    int shape, int chunks_per_xcd,
    const ProblemDesc *__restrict__ probs, const PoseState *__restrict__ poses,
    double *__restrict__ partials, int lds_texels) {
  eval_fused_body<T, PPT, MODE, NT, VAR, BUF, IMG32, true>(x0, y0, z0, n0, shape, chunks_per_xcd, probs, poses, partials, lds_texels);
}
template <typename T, int PPT, int MODE, int NT, bool VAR, bool BUF, bool IMG32 = false>
__global__ __launch_bounds__(NT) void ea_eval_poses_grid_w_kernel(
    const void *__restrict__ x0, const void *__restrict__ y0, const void *__restrict__ z0, int n0,
    int shape, int chunks_per_xcd,
    const ProblemDesc *__restrict__ probs, const PoseState *__restrict__ poses,
    double *__restrict__ partials, int lds_texels) {
  eval_fused_body<T, PPT, MODE, NT, VAR, BUF, IMG32, true>(x0, y0, z0, n0, shape, chunks_per_xcd, probs, poses, partials, lds_texels);
}
#endif

#ifndef EA_TU_VARIANT
// ------------------------------------------------------------------------------------------------
// per-point outputs (parity / "EAResidue batch Evaluate" view): r[n], J[n*6]

template <typename T>
__global__ __launch_bounds__(kBlockThreads) void ea_eval_points_kernel(
    const ProblemDesc *__restrict__ probs, int problem, const PoseState *__restrict__ poses,
    double *__restrict__ r_out, double *__restrict__ J_out, int corrected) {
  const ProblemDesc &pd = probs[problem];
  const PoseState &ps = poses[pd.group];
  const int i = blockIdx.x * kBlockThreads + threadIdx.x;
  if (i >= pd.n) return;
  const T x = static_cast<const T *>(pd.x)[i], y = static_cast<const T *>(pd.y)[i], z = static_cast<const T *>(pd.z)[i];
  const double nan = __builtin_nan("");
  if (pd.variant) {  // distortion / second-camera functors
    ProjV<T> pv;
    project_point_var<T>(pd, ps, x, y, z, pv);
    if (pv.state != 1) {
      if (r_out) r_out[i] = nan;
      if (J_out)
        for (int a = 0; a < 6; ++a) J_out[(size_t)i * 6 + a] = nan;
      return;
    }
    const int pitchv = pd.pitch;
    const T *basev = static_cast<const T *>(pd.dt) + (size_t)kImagePad * (size_t)pitchv + kImagePad +
                     (ptrdiff_t)(pv.iv - 1) * pitchv + (pv.iu - 1);
    T f, Fu, Fv;
    bicubic<T>(pv.fu, pv.fv, [&](int l) { return *reinterpret_cast<const Row4<T> *>(basev + (ptrdiff_t)l * pitchv); }, f, Fu, Fv);
    T J[6];
    jacobian_row_var<T>(pd, ps, pv, Fu, Fv, J);
    T sc = T(1);
    if (corrected) {
      T rho, w;
      loss_eval<T>(pd.loss_kind, Uni<T>::loss_a(pd), Uni<T>::loss_inv_b(pd), f * f, rho, w);
      if (const T *wts = desc_weights<T>(pd, i)) w *= *wts;  // ScaledLoss: sqrt(w_i rho')
      sc = t_sqrt<T>(w);
    }
    if (r_out) r_out[i] = (double)(sc * f);
    if (J_out)
      for (int a = 0; a < 6; ++a) J_out[(size_t)i * 6 + a] = (double)(sc * J[a]);
    return;
  }
  Proj<T> pr;
  project_point<T>(pd, ps, x, y, z, pr);
  if (pr.state != 1) {
    if (r_out) r_out[i] = nan;
    if (J_out)
      for (int a = 0; a < 6; ++a) J_out[(size_t)i * 6 + a] = nan;
    return;
  }
  const int pitch = pd.pitch;
  const T *base = static_cast<const T *>(pd.dt) + (size_t)kImagePad * (size_t)pitch + kImagePad +
                  (ptrdiff_t)(pr.iv - 1) * pitch + (pr.iu - 1);
  T f, Fu, Fv;
  bicubic<T>(pr.fu, pr.fv, [&](int l) { return *reinterpret_cast<const Row4<T> *>(base + (ptrdiff_t)l * pitch); }, f, Fu, Fv);
  T J[6];
  jacobian_row<T>(pd, ps, pr, x, y, z, Fu, Fv, J);
  T sc = T(1);
  if (corrected) {
    T rho, w;
    loss_eval<T>(pd.loss_kind, Uni<T>::loss_a(pd), Uni<T>::loss_inv_b(pd), f * f, rho, w);
    if (const T *wts = desc_weights<T>(pd, i)) w *= *wts;
    sc = t_sqrt<T>(w);
  }
  if (r_out) r_out[i] = (double)(sc * f);
  if (J_out)
    for (int a = 0; a < 6; ++a) J_out[(size_t)i * 6 + a] = (double)(sc * J[a]);
}

// ------------------------------------------------------------------------------------------------
// Materialised mode (the "EAResidue batch Evaluate" view): residual and 1x6 row of EVERY point written out in
// the problem's arithmetic type -- what N calls of AutoDiffCostFunction<EAResidue,1,4,3>::Evaluate followed by the
// parameterisation's 4x3 plus-Jacobian produce (standalone/utils.h:48-92, standalone_edge_align.cpp:271-278), for a caller
// that runs its own solver on the rows.  One point per lane, 256-lane workgroups, the chunk -> XCD mapping and the
// raw-buffer stencil loads of the fused kernel, no reduction.  Unlike the fused mode this one IS bandwidth-bound:
// 3 s bytes in and 7 s bytes out per point plus one pass over the DT image (s = sizeof(T)).
//   LAYOUT 0: J row-major [rows][6] (what Ceres hands its linear solver); the 6 values of a lane are 24 / 48 contiguous
//             bytes, so a wavefront's 64 rows go through an LDS transpose and leave as three stores of 64 x 8 / 16
//             contiguous bytes (STAGED; the direct form -- three 8/16-byte stores per lane at a 24/48-byte stride -- is kept
//             for comparison);
//   LAYOUT 1: J column-major [6][total rows] (six coalesced stores, no staging).
// Rows of a functor that returned false are NaN (and counted): Ceres fails the whole evaluation in that case.
// `corrected`: rows scaled by sqrt(rho'(r^2)) (Ceres' Corrector with alpha = 0, as the fused mode accumulates them).
template <typename T> struct PairOf;
template <> struct PairOf<float> { typedef float type __attribute__((ext_vector_type(2))); };
template <> struct PairOf<double> { typedef double type __attribute__((ext_vector_type(2))); };
template <typename T> using Pair = typename PairOf<T>::type;  // two consecutive elements: one 8- / 16-byte access

#ifndef EA_ROWS_WAVES_F64
#define EA_ROWS_WAVES_F64 4  // (fp64 occupancy target of the rows kernel, wavefronts per SIMD: A/B knob, scripts/archive/ab_rows.sh)
#endif
template <typename T, bool VAR, bool BUF, int LAYOUT, bool STAGED, bool IMG32 = false>
__global__ __launch_bounds__(kBlockThreads) __attribute__((amdgpu_waves_per_eu(sizeof(T) == 8 ? EA_ROWS_WAVES_F64 : 8, 8)))
void ea_eval_rows_kernel(
    const ProblemDesc *__restrict__ probs, const PoseState *__restrict__ poses, int chunks_per_xcd, int corrected, int nontemporal,
    long long total_rows, T *__restrict__ r_out, T *__restrict__ J_out, unsigned int *__restrict__ n_invalid) {
  constexpr int NT = kBlockThreads;
  const int bx = blockIdx.x;
  const int c = (bx & 7) * chunks_per_xcd + (bx >> 3);
  const ProblemDesc pd = probs[blockIdx.y];
  const long long start = (long long)c * NT;
  if (start >= pd.n) return;  // (uniform)
  const PoseState *psp = poses + pd.group;
  PoseLite<T> ps;
  {
    const T *R_ = Uni<T>::R(*psp), *t_ = Uni<T>::t(*psp);
#pragma unroll
    for (int i = 0; i < 9; ++i) ps.R[i] = R_[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) ps.t[i] = t_[i];
    ps.unit_q = psp->unit_q;
    ps.full = psp;
  }
  const int count = min(NT, (int)(pd.n - start));
  const int tid = threadIdx.x;
  const int j = min(tid, count - 1);  // lanes past the end re-read the chunk's last point and store nothing
  const bool inb = tid < count;
  T X, Y, Z;
  if constexpr (BUF) {
    const __amdgpu_buffer_rsrc_t rx = make_raw_buffer(static_cast<const T *>(pd.x) + start, (unsigned)count * (unsigned)sizeof(T));
    const __amdgpu_buffer_rsrc_t ry = make_raw_buffer(static_cast<const T *>(pd.y) + start, (unsigned)count * (unsigned)sizeof(T));
    const __amdgpu_buffer_rsrc_t rz = make_raw_buffer(static_cast<const T *>(pd.z) + start, (unsigned)count * (unsigned)sizeof(T));
    const int poff = j * (int)sizeof(T);
    X = buf_load_elem<T>(rx, poff); Y = buf_load_elem<T>(ry, poff); Z = buf_load_elem<T>(rz, poff);
  } else {
    X = static_cast<const T *>(pd.x)[start + j]; Y = static_cast<const T *>(pd.y)[start + j]; Z = static_cast<const T *>(pd.z)[start + j];
  }
  const int pitch = pd.pitch;
  T f, Fu, Fv, J[6];
  int state;
  static_assert(!IMG32 || (std::is_same<T, double>::value && !VAR), "fp32-stored image: plain fp64 kernels");
  typedef typename ImgOf<T, IMG32>::type IT;
  const void *img_base = IMG32 ? pd.dt32 : pd.dt;
  auto sample = [&](int iu, int iv, T fu, T fv) {
    if constexpr (BUF) {
      const __amdgpu_buffer_rsrc_t rimg = make_raw_buffer(img_base, (unsigned)pitch * (unsigned)(pd.H + 2 * kImagePad) * (unsigned)sizeof(IT));
      const int voff = ((iv + (kImagePad - 1)) * pitch + (iu + (kImagePad - 1))) * (int)sizeof(IT);
      bicubic<T>(fu, fv, [&](int l) { return RowLoad<T, IT>::buf(rimg, voff, l * pitch * (int)sizeof(IT)); }, f, Fu, Fv);
    } else {
      const GPtr<IT> base = (GPtr<IT>)(static_cast<const IT *>(img_base) + (size_t)kImagePad * (size_t)pitch + kImagePad) +
                            ((ptrdiff_t)(iv - 1) * pitch + (iu - 1));
      bicubic<T>(fu, fv, [&](int l) { return RowLoad<T, IT>::flat(base + (ptrdiff_t)l * pitch); }, f, Fu, Fv);
    }
  };
  if constexpr (VAR) {
    ProjV<T> pv;
    project_point_var<T>(pd, ps, X, Y, Z, pv);
    state = pv.state;
    sample(pv.iu, pv.iv, pv.fu, pv.fv);
    jacobian_row_var<T>(pd, ps, pv, Fu, Fv, J);
  } else {
    Proj<T> pr;
    project_point<T>(pd, ps, X, Y, Z, pr);
    state = pr.state;
    sample(pr.iu, pr.iv, pr.fu, pr.fv);
    jacobian_row<T>(pd, ps, pr, X, Y, Z, Fu, Fv, J);
  }
  T sc = T(1);
  if (corrected) {  // (uniform)
    T rho, w;
    loss_eval<T>(pd.loss_kind, Uni<T>::loss_a(pd), Uni<T>::loss_inv_b(pd), f * f, rho, w);
    if constexpr (VAR) {  // (a weighted term is a variant: the plain instantiations never meet one)
      if (const T *wts = desc_weights<T>(pd, start + j)) w *= *wts;
    }
    sc = t_sqrt<T>(w);
  }
  const bool bad = state == 2;
  if (__any(bad)) {  // (uniform test first: the common wavefront has nothing to mark)
    if (bad) {
      sc = (T)__builtin_nan("");
      f = T(1);
#pragma unroll
      for (int a = 0; a < 6; ++a) J[a] = T(1);
      if (inb) atomicAdd(n_invalid, 1u);
    }
  }
  f *= sc;
#pragma unroll
  for (int a = 0; a < 6; ++a) J[a] *= sc;
  const long long row0 = pd.row_begin + start;  // first row of this workgroup
  auto put = [&](T *p, T v) { if (nontemporal) __builtin_nontemporal_store(v, p); else *p = v; };
  if (inb) put(r_out + row0 + tid, f);
  if constexpr (LAYOUT == 1) {
    if (inb) {
#pragma unroll
      for (int a = 0; a < 6; ++a) put(J_out + (long long)a * total_rows + row0 + tid, J[a]);
    }
  } else if constexpr (!STAGED) {
    if (inb) {
      Pair<T> *dst = reinterpret_cast<Pair<T> *>(J_out + (row0 + tid) * 6);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        Pair<T> v;
        v.x = J[2 * k]; v.y = J[2 * k + 1];
        if (nontemporal) __builtin_nontemporal_store(v, dst + k); else dst[k] = v;
      }
    }
  } else {
    // wavefront-local transpose: lane l writes its 6 values at [6 l .. 6 l + 5] of the wavefront's 384-element strip, then
    // reads elements (2 l, 2 l + 1) + 128 k, k = 0..2, and stores them: each store instruction of the wavefront covers
    // 64 x 2 consecutive elements.  LDS operations of one wavefront complete in order; nothing else touches the strip.
    __shared__ __align__(16) T s_rows[(NT / 64) * 384];
    const int lane = tid & 63, wave = tid >> 6;
    T *strip = s_rows + wave * 384;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      Pair<T> v;
      v.x = J[2 * k]; v.y = J[2 * k + 1];
      *reinterpret_cast<Pair<T> *>(strip + 6 * lane + 2 * k) = v;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int valid = 6 * max(0, min(64, count - 64 * wave));  // elements of the strip that belong to real points
    T *dst = J_out + (row0 + 64 * wave) * 6;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int e = 2 * lane + 128 * k;
      const Pair<T> v = *reinterpret_cast<const Pair<T> *>(strip + e);
      if (e < valid) {
        if (nontemporal) __builtin_nontemporal_store(v, reinterpret_cast<Pair<T> *>(dst + e)); else *reinterpret_cast<Pair<T> *>(dst + e) = v;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// The reference's own quantitative self-check (standalone_edge_align.cpp:2494-2567 before the solve, :2704-2776 after):
// every point warped by the pose, divided by its depth, pushed through K, truncated `(int)` to a pixel, the distance
// transform read at that pixel; total, maximum and where the maximum sits.  One partial per workgroup
// {sum, max, u of max, v of max, smallest point index holding the max, points inside, points outside}; the host folds
// them in workgroup order.  Arithmetic is fp64 with the reference's operation order (x / z first, then fx * x + cx, no
// contraction) so that borderline pixels truncate the same way.  Upstream reads outside the image without a check
// (undefined behaviour); such points are skipped here and counted.
struct PixelCostPartial {
  double sum, max, max_u, max_v;
  long long max_index, inside, outside;
  long long pad_;
};

template <typename T>
__global__ __launch_bounds__(kBlockThreads) void ea_pixel_cost_kernel(const ProblemDesc *__restrict__ probs, int problem,
                                                                      const PoseState *__restrict__ poses,
                                                                      PixelCostPartial *__restrict__ out) {
  __shared__ double s_sum[kBlockThreads / 64], s_max[kBlockThreads / 64], s_u[kBlockThreads / 64], s_v[kBlockThreads / 64];
  __shared__ long long s_idx[kBlockThreads / 64], s_in[kBlockThreads / 64], s_out[kBlockThreads / 64];
  const ProblemDesc &pd = probs[problem];
  const PoseState &ps = poses[pd.group];
  const int i = blockIdx.x * kBlockThreads + threadIdx.x;
  double cost = 0.0, mx = -1.0, mu = 0.0, mv = 0.0;  // upstream starts MaxCost at -1
  long long midx = 0x7fffffffffffffffLL, nin = 0, nout = 0;
  if (i < pd.n) {
    const double x = (double)static_cast<const T *>(pd.x)[i], y = (double)static_cast<const T *>(pd.y)[i],
                 z = (double)static_cast<const T *>(pd.z)[i];
    const double *R = ps.R, *t = ps.t;
    // Eigen's 4x4 * 4x1 product, row by row, left to right; then x / z, fx * x + cx.  No contraction: upstream's build
    // has no FMA, and fma(fy, y / z, cy) lands on 34.999999999999986 where the two roundings give 35.0 -- another pixel.
    // (hipcc contracts __dmul_rn + __dadd_rn pairs like plain operators, hence the pragma.)
    double bx, by, bz, u, v;
    {
#pragma clang fp contract(off)
      bx = ((R[0] * x + R[1] * y) + R[2] * z) + t[0];
      by = ((R[3] * x + R[4] * y) + R[5] * z) + t[1];
      bz = ((R[6] * x + R[7] * y) + R[8] * z) + t[2];
      const double xn = bx / bz, yn = by / bz;
      u = pd.fx * xn + pd.cx;
      v = pd.fy * yn + pd.cy;
    }
    const bool finite = (u == u) && (v == v) && fabs(u) < 1e9 && fabs(v) < 1e9;
    const int iu = finite ? (int)u : -1, iv = finite ? (int)v : -1;  // `(int)`: truncation toward zero
    if (finite && iu >= 0 && iu < pd.W && iv >= 0 && iv < pd.H && !(u <= -1.0) && !(v <= -1.0)) {
      cost = (double)static_cast<const T *>(pd.dt)[(size_t)(iv + kImagePad) * (size_t)pd.pitch + (size_t)(iu + kImagePad)];
      mx = cost; mu = u; mv = v; midx = i; nin = 1;
    } else {
      nout = 1;
    }
  }
  // wavefront reduction: sum, count, and (max, smallest index) with the pixel carried along
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    cost += __shfl_xor(cost, m, 64);
    nin += __shfl_xor(nin, m, 64);
    nout += __shfl_xor(nout, m, 64);
    const double omx = __shfl_xor(mx, m, 64), ou = __shfl_xor(mu, m, 64), ov = __shfl_xor(mv, m, 64);
    const long long oi = __shfl_xor(midx, m, 64);
    if (omx > mx || (omx == mx && oi < midx)) { mx = omx; mu = ou; mv = ov; midx = oi; }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { s_sum[wave] = cost; s_max[wave] = mx; s_u[wave] = mu; s_v[wave] = mv; s_idx[wave] = midx; s_in[wave] = nin; s_out[wave] = nout; }
  __syncthreads();
  if (threadIdx.x == 0) {
    PixelCostPartial o;
    o.sum = 0.0; o.max = -1.0; o.max_u = 0.0; o.max_v = 0.0; o.max_index = 0x7fffffffffffffffLL; o.inside = 0; o.outside = 0; o.pad_ = 0;
    for (int w = 0; w < kBlockThreads / 64; ++w) {
      o.sum += s_sum[w]; o.inside += s_in[w]; o.outside += s_out[w];
      if (s_max[w] > o.max || (s_max[w] == o.max && s_idx[w] < o.max_index)) { o.max = s_max[w]; o.max_u = s_u[w]; o.max_v = s_v[w]; o.max_index = s_idx[w]; }
    }
    out[blockIdx.x] = o;
  }
}

// ------------------------------------------------------------------------------------------------
// fixed-order reduction of a problem's tile partials -> 32 accumulators

constexpr int kFoldThreads = 1024;  // plain fold: 32 slots x 32 strided groups
constexpr int kLmThreads = 256;     // fold + scalar LM code: 4 waves = one per SIMD, so the scalar code can keep
                                    // its ~300 live registers without spilling to scratch

// LDS doubles reduce_tiles needs for a workgroup of NTHREADS threads
template <int NTHREADS> constexpr int reduce_tiles_lds() { return (NTHREADS / 16 + NTHREADS / 256) * kAccSlots; }

// A row is 32 doubles = 256 bytes.  Lanes fetch 16 bytes each (two slots): 16 lanes cover a row, a wavefront four rows per
// load instruction.  (With 8 bytes per lane the fold of 196 rows was 128 wave-level load instructions through the one
// texture-address unit of the CU at ~20 cycles each -- the instruction count, not the latency of the round trip, was what
// the LM step waited for: in-kernel stamps, 4.7 k cycles for the fold.)  Thread (id, j) = (tid & 15, tid >> 4) sums slots
// 2 id, 2 id + 1 of rows begin + j + u G, u = 0 .. U-1, G = NTHREADS / 16 row groups, round after round of U G rows.
template <int NTHREADS, int U>
__device__ __forceinline__ void reduce_tiles(const double *__restrict__ partials, int tile_begin,
                                             int tile_end, double *s_part /* reduce_tiles_lds<NTHREADS>() */,
                                             double *out /* 32, threads 0..31 write */) {
  constexpr int G = NTHREADS / 16, F = NTHREADS / 256;
  static_assert(U == 4 || U == 8, "pairwise combine below");
  static_assert(NTHREADS == 256 || NTHREADS == 1024, "final stage: 16 groups per thread");
  typedef double D2 __attribute__((ext_vector_type(2)));
  const int tid = threadIdx.x;
  const int id = tid & 15, j = tid >> 4;
  // fixed summation order for a given tile count; 2 U independent loads in flight per thread
  D2 s[U];
#pragma unroll
  for (int u = 0; u < U; ++u) s[u] = D2{0.0, 0.0};
  // A round = U rows per lane.  Rows past the end are loaded from the last row (a valid address) and masked out
  // of the sum, so a round is U back-to-back loads with no branches; the first two rounds are issued together:
  // folds of up to 2 U G rows cost one memory round trip.
  const int last = tile_end - 1;
  if (tile_begin <= last) {  // uniform
    auto load_round = [&](int base, D2(&v)[U]) {
#pragma unroll
      for (int u = 0; u < U; ++u)
        v[u] = *reinterpret_cast<const D2 *>(partials + (size_t)min(base + j + u * G, last) * kAccSlots + 2 * id);
    };
    auto add_round = [&](int base, const D2(&v)[U]) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool in = base + j + u * G <= last;
        s[u].x += in ? v[u].x : 0.0;
        s[u].y += in ? v[u].y : 0.0;
      }
    };
    D2 v0[U], v1[U];
    load_round(tile_begin, v0);
    if (tile_begin + U * G <= last) {  // uniform
      load_round(tile_begin + U * G, v1);
      add_round(tile_begin, v0);
      add_round(tile_begin + U * G, v1);
      for (int base = tile_begin + 2 * U * G; base <= last; base += U * G) {
        load_round(base, v0);
        add_round(base, v0);
      }
    } else {
      add_round(tile_begin, v0);
    }
  }
#pragma unroll
  for (int w = 1; w < U; w *= 2)
#pragma unroll
    for (int u = 0; u + w < U; u += 2 * w) s[u] += s[u + w];
  *reinterpret_cast<D2 *>(s_part + j * kAccSlots + 2 * id) = s[0];
  __syncthreads();
  // final stage: slot `tid & 31` over 16 row groups per thread, in group order; with 1024 threads four such partial sums per
  // slot, combined in order by the first 32 threads
  if constexpr (F == 1) {
    if (tid < kAccSlots) {
      double tot = 0.0;
#pragma unroll
      for (int k = 0; k < G; ++k) tot += s_part[k * kAccSlots + tid];
      out[tid] = tot;
    }
  } else {
    double *s_fin = s_part + G * kAccSlots;
    if (tid < kAccSlots * F) {
      const int slot = tid & 31, f = tid >> 5;
      double tot = 0.0;
#pragma unroll
      for (int k = 0; k < 16; ++k) tot += s_part[(16 * f + k) * kAccSlots + slot];
      s_fin[f * kAccSlots + slot] = tot;
    }
    __syncthreads();
    if (tid < kAccSlots) {
      double tot = 0.0;
#pragma unroll
      for (int f = 0; f < F; ++f) tot += s_fin[f * kAccSlots + tid];
      out[tid] = tot;
    }
  }
}

__global__ __launch_bounds__(kFoldThreads) void ea_reduce_kernel(const GroupDesc *__restrict__ groups,
                                                                  const double *__restrict__ partials,
                                                                  EvalOut *__restrict__ out) {
  __shared__ __align__(16) double s_part[reduce_tiles_lds<kFoldThreads>()];
  const GroupDesc gd = groups[blockIdx.x];
  reduce_tiles<kFoldThreads, 4>(partials, gd.tile_begin, gd.tile_end, s_part, out[blockIdx.x].acc);
}

// One workgroup of a launch of n is done: its lane 0 makes the workgroup's stores visible system-wide (the fence waits for the
// wavefront's stores) and counts itself in; the last arrival re-arms the counter and raises the flag in pinned host memory
// to the launch's sequence number (release, system scope).  Call from lane 0 of the wavefront that stored.
__device__ __forceinline__ void signal_done(unsigned int *counter, unsigned int n, int *host_flag, int seq) {
  __threadfence_system();
  const unsigned int prev = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
  if (prev == n - 1u) {
    __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence_system();
    __hip_atomic_store(host_flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// The same fold for the synchronous evaluations (ea_batch_eval, ea_batch_eval_poses), whose results go straight into pinned
// host memory: the workgroup that finishes last raises a flag there, so that the host can poll for "every result has
// landed" instead of waiting for the stream's completion signal (~10 us later).  Every workgroup's 32 result words are
// stored by its wavefront 0; lane 0 of that wavefront makes them visible system-wide (the fence waits for the wavefront's
// stores), then counts itself in; the workgroup that completes the count re-arms the counter and raises the flag to
// `seq` (release, system scope).  Launches on one stream execute in order: earlier folds of the same call are complete.
__global__ __launch_bounds__(kFoldThreads) void ea_reduce_done_kernel(const GroupDesc *__restrict__ groups,
                                                                       const double *__restrict__ partials,
                                                                       EvalOut *__restrict__ out, unsigned int *__restrict__ counter,
                                                                       int *__restrict__ host_flag, int seq) {
  __shared__ __align__(16) double s_part[reduce_tiles_lds<kFoldThreads>()];
  const GroupDesc gd = groups[blockIdx.x];
  reduce_tiles<kFoldThreads, 4>(partials, gd.tile_begin, gd.tile_end, s_part, out[blockIdx.x].acc);
  if (threadIdx.x == 0) signal_done(counter, gridDim.x, host_flag, seq);
}

// The fold as a 256-thread workgroup sums it when it rides in an evaluation launch (ea_eval_fold_kernel below; 8 rows in
// flight per lane keep the riding workgroup inside the evaluation's register budget): closes a pipelined sequence.
__global__ __launch_bounds__(kLmThreads) void ea_reduce256_kernel(const GroupDesc *__restrict__ groups,
                                                                  const double *__restrict__ partials,
                                                                  EvalOut *__restrict__ out) {
  __shared__ __align__(16) double s_part[reduce_tiles_lds<kLmThreads>()];
  const GroupDesc gd = groups[blockIdx.x];
  reduce_tiles<kLmThreads, 4>(partials, gd.tile_begin, gd.tile_end, s_part, out[blockIdx.x].acc);
}

// Evaluation k with the fold of evaluation k-1 riding in the same launch: one extra workgroup per problem (the last
// column of the grid) folds the rows the PREVIOUS launch left in `prev_rows` into `prev_out` while the others evaluate
// into `partials` (a different row array).  A stream of independent evaluations then costs one launch per evaluation
// instead of two dependent ones -- the fold's kernel boundary (1.45 us) and its memory round trip disappear under the
// evaluation.  The fold workgroup sums in the order reduce_tiles<NT> gives a workgroup of this size.
// Plain single-family problems, stencil rows from L2 (MODE 0).
template <typename T, int PPT, int NT, bool BUF, bool IMG32 = false>
__global__ __launch_bounds__(NT) void ea_eval_fold_kernel(
    const void *__restrict__ x0, const void *__restrict__ y0, const void *__restrict__ z0, int n0,
    int shape, int chunks_per_xcd,
    const ProblemDesc *__restrict__ probs, const PoseState *__restrict__ poses,
    double *__restrict__ partials, int lds_texels,
    const GroupDesc *__restrict__ groups, const double *__restrict__ prev_rows, EvalOut *__restrict__ prev_out) {
  if (blockIdx.x == gridDim.x - 1) {  // (uniform)
    __shared__ __align__(16) double s_part[reduce_tiles_lds<NT>()];
    const GroupDesc gd = groups[blockIdx.y];
    reduce_tiles<NT, 4>(prev_rows, gd.tile_begin, gd.tile_end, s_part, prev_out[blockIdx.y].acc);
    return;
  }
  eval_fused_body<T, PPT, 0, NT, false, BUF, IMG32>(x0, y0, z0, n0, shape, chunks_per_xcd, probs, poses, partials, lds_texels);
}

// One result of a pose-batched launch folded by one workgroup of NT threads, in the order reduce_tiles<NT, 4> gives a
// workgroup of this size -- riding in the next evaluation launch or in the stand-alone fold that closes a call, the same
// sums.  Wavefront 0 stores the 32 words; its lane 0 makes them visible system-wide, counts itself in, and the last
// arrival of the launch re-arms the counter and raises the pinned flag to the launch's sequence number.
template <int NT>
__device__ __forceinline__ void poses_fold_one(const PosesFold &f, int r) {
  __shared__ __align__(16) double s_part[reduce_tiles_lds<NT>()];
  int pose, problem;
  poses_rider(r, f.count, &pose, &problem);
  const GroupDesc gd = f.groups[problem];
  const int base = pose * f.rows_per_pose;
  reduce_tiles<NT, 4>(f.rows, base + gd.tile_begin, base + gd.tile_end, s_part, f.out[r].acc);
  if (threadIdx.x == 0) signal_done(f.counter, (unsigned)f.n, f.host_flag, f.seq);
}

// The pose-batched evaluation of the plain functor on the L2 path: g poses of a batch in ONE one-dimensional launch whose
// work items -- (row of a pose, pose) pairs -- are dealt evenly over the 8 XCDs (ea_poses_map.h), with the fold of the
// PREVIOUS launch's rows riding in front.  A short head of its own in front of the unchanged fused_chunk: chunks, per-point
// code, reductions and the row index pose * rows + row are those of the (chunks, G x terms) grid it replaces, so every
// partial row holds the same bits.  The first 14 dwords still arrive with the wave: term 0's points and count, the packed
// shape, g and rows, the descriptor and pose tables -- all an item of a single-term batch needs to find its pose, its
// descriptor and its points without a dependent load, at EVERY pose (the 2-D grid issued the early point loads for pose 0
// only).  A batch of several terms reads one 16-byte entry of the row table first; the table sits right in front of the
// descriptors (probs - rows entries), so that no further pointer has to be fetched for it.
template <typename T, int PPT, int MODE, int NT, bool VAR, bool BUF, bool IMG32 = false>
__global__ __launch_bounds__(NT) void ea_eval_poses_kernel(
    const void *__restrict__ x0, const void *__restrict__ y0, const void *__restrict__ z0, int n0,
    int shape, int g, int rows,
    const ProblemDesc *__restrict__ probs, const PoseState *__restrict__ poses,
    double *__restrict__ partials, PosesFold fold) {
  static_assert((MODE == 0 || MODE == kModeExchange) && !VAR, "plain functor, stencil rows from L2");
  constexpr bool XCHG = MODE == kModeExchange;
  extern __shared__ __align__(16) unsigned char smem[];
  double *s_red = reinterpret_cast<double *>(smem);
  int *s_box = reinterpret_cast<int *>(smem + kRedBytes);
  const PosesWork w = poses_work(blockIdx.x, shape, rows, g, fold.n);
  if (w.kind != 2) {  // (uniform)
    if (w.kind == 1) poses_fold_one<NT>(fold, w.rider);
    return;
  }
  const PosesChunk pc = poses_chunk(w, shape, rows, reinterpret_cast<const PosesRow *>(probs) - rows);
  const int tid = threadIdx.x;
  EA_ITEM_HEAD(false, NT * PPT, pc.chunk, pc.term, pc.slot, false, return);
  const double sum = fused_chunk<T, PPT, 0, NT, false, BUF, IMG32, PoseLite<T>, XCHG>(pd, ps, X, Y, Z, count, s_red, s_box, (T *)nullptr, 0,
                                                                                       tid < kAccSlots ? tid : -1);
  store_row_sum<XCHG>(partials, pc.out_row, sum);
}

// the fold that closes a call of the pose-batched path: the last launch's rows, as its riders would have folded them
template <int NT>
__global__ __launch_bounds__(NT) void ea_poses_fold_kernel(PosesFold fold) {
  poses_fold_one<NT>(fold, blockIdx.x);
}

// ---- the pose-batched fp64 evaluation with one pose per LANE ---------------------------------------------------------------
// ea_eval_poses_kernel maps lanes to points, so each of its 28 sums crosses lanes -- exchange buffer, barriers and butterfly
// per 512 (point, pose) pairs.  A call of many poses has a second long axis: here a lane owns a POSE (its twelve constants
// in vector registers) and the wavefront walks points, which are wave-uniform and arrive through scalar loads.  Every sum
// and the failed-functor count stay inside their lane from the first point to the last; nothing crosses lanes and no
// barrier stands in the point loop.  A work item is (row of a pose, 64 consecutive poses of the launch) (ea_poses_map.h); the
// row is the 512-point chunk it is in the other kernel.  Its sums go lane-minor into the path's own row array and are folded
// inside the launch (further down).  The workgroup's four wavefronts hold the same 64 poses and walk the chunk's four sub-runs of 128
// points, two points per iteration, sums in the order of the points (under the unweighted Cauchy loss of unit quaternions
// the cost is ONE logarithm per sub-run, of the running product of the points' factors: lanes_sums); at the end the
// per-lane sums are added through LDS as (w0 + w1) + (w2 + w3) and lane l stores the row of pose l.  The summation order differs from the other kernel's (last places), and depends on nothing but the pose and the
// row: not on the lane, the company in the wavefront, the launch or the item order.  The per-point expressions are fused_chunk's, through the same
// functions; lanes whose pose is not a unit quaternion, or whose point fails, take their branch per lane.
template <typename T> using CPtr = const T __attribute__((address_space(4))) *;  // read-only for the kernel: uniform loads go through the scalar cache
constexpr int kLanesWaves = 4, kLanesSub = 512 / kLanesWaves, kLanesVals = 29;  // (28 sums + failed functors)

// What a lane keeps of a point between asking for its stencil rows and summing it up: the rows as loaded (an fp32-stored image
// stays fp32 until it is used) and six words of the projection.  The other five (bx, by, fxz, fyz and the fix-up of a lane
// without a valid point) are formed again from these by project_point's own expressions when the point is summed: four
// instructions instead of ten registers held across the loads.
template <typename IT> struct LanesStage {
  double cx_, cy_, cz_, iz, fu, fv;
  unsigned long long bad;  // the lanes without a valid point, as a mask in scalar registers (lanes_any / lanes_mine)
  Row4<IT> row[4];
};
// "Some lane has no valid point", made once per point where the mask is formed and asked again where a fix-up stands: a scalar
// compare and a scalar branch.  (The mask goes through an empty asm: where the compiler sees the ballot behind the test it
// keeps the lanes' flag in a vector register instead and compares that again at every site.)
__device__ __forceinline__ bool lanes_any(unsigned long long &m) {
  asm volatile("" : "+s"(m));
  return m != 0;
}
__device__ __forceinline__ bool lanes_mine(unsigned long long m) { return __builtin_amdgcn_inverse_ballot_w64(m); }
template <typename IT> __device__ __forceinline__ Row4<double> lanes_widen(const Row4<IT> &r) {
  Row4<double> o;
  o.p0 = (double)r.p0; o.p1 = (double)r.p1; o.p2 = (double)r.p2; o.p3 = (double)r.p3;
  return o;
}
// Stage 1 of a point: project, count a failed functor, move the lanes without a valid point to a harmless sample, and issue
// the four row loads.  inb (uniform): the point exists -- an odd sub-run ends on a copy of its last point.
template <bool BUF, bool IMG32>
__device__ __forceinline__ void lanes_stage(const ProblemDesc &pd, const PoseLite<double> &ps, double x, double y, double z,
                                            bool inb, LanesStage<typename ImgOf<double, IMG32>::type> &st, int &n_bad) {
  typedef double T;
  typedef typename ImgOf<T, IMG32>::type IT;
  const int pitch = pd.pitch;
  const void *img_base = IMG32 ? pd.dt32 : pd.dt;
  Proj<T> pr;
  project_point<T>(pd, ps, x, y, z, pr);
  const bool valid = inb && pr.state == 1;
  n_bad += (inb && pr.state == 2) ? 1 : 0;
  st.bad = __builtin_amdgcn_ballot_w64(!valid);
  if (lanes_any(st.bad)) {  // (uniform test first, as in fused_chunk)
    asm volatile("" ::: "memory");  // (and kept a branch, as in jacobian_row)
    if (lanes_mine(st.bad)) { pr.iu = 0; pr.iv = 0; pr.fu = T(0); pr.fv = T(0); }
  }
  st.cx_ = pr.cx_; st.cy_ = pr.cy_; st.cz_ = pr.cz_; st.iz = pr.iz; st.fu = pr.fu; st.fv = pr.fv;
  if constexpr (BUF) {
    const __amdgpu_buffer_rsrc_t rimg =
        make_raw_buffer(img_base, (unsigned)pitch * (unsigned)(pd.H + 2 * kImagePad) * (unsigned)sizeof(IT));
    const int voff = ((pr.iv + (kImagePad - 1)) * pitch + (pr.iu + (kImagePad - 1))) * (int)sizeof(IT);
#pragma unroll
    for (int l = 0; l < 4; ++l) st.row[l] = buf_load_row4<IT>(rimg, voff, l * pitch * (int)sizeof(IT));
  } else {
    const GPtr<IT> gimg = (GPtr<IT>)(static_cast<const IT *>(img_base) + (size_t)kImagePad * (size_t)pitch + kImagePad);
    const GPtr<IT> base = gimg + ((ptrdiff_t)(pr.iv - 1) * pitch + (pr.iu - 1));
#pragma unroll
    for (int l = 0; l < 4; ++l) st.row[l] = load_row4<IT>(base + (ptrdiff_t)l * pitch);
  }
}
// Stage 2: staged point k of its pair into the lane's sums, fused_chunk's statements.  UNIT: every lane's pose is a unit
// quaternion (the test is made once per work item), else each lane takes its own branch of jacobian_row.
//
// The cost under the unweighted Cauchy loss (`pair`) of the UNIT form: the lane needs sum log s_i over the 128 points of its
// sub-run, which is log prod s_i -- so a point only multiplies its factor s = 1 + r^2 / a^2 (exactly 1 for a lane without a
// valid point) into the lane's running product `run` (pl_run_*, ea_pair_log.h: a multiply and two fmas that carry the rounding
// error along, one comparison that guards the range) and lanes_run takes one logarithm behind the loop, where the paired
// logarithm cost ~22 instructions per point.  w = 1 / s stays per point: JtJ, Jtr and the failed-functor count keep their
// bits, the cost moves in its last places.  Huber, the trivial loss and the general-quaternion form keep loss_point and
// cost_point, the paired logarithm included.
//
// Every fix-up of a lane without a valid point, and the renormalisation of the product, is a uniform BRANCH (the empty asm, as
// in jacobian_row): written as `__any(c) && c` alone the compiler turns them into moves under an exec mask, which every
// wavefront issues for every point.  `cost` and `held` are touched behind such a branch as well: the unit Cauchy path spends no
// instruction on them.
//
// `under` is called right behind bx, by and their fix-up, in front of the sixteen taps: what the caller issues there (the next
// pair's coordinates, lanes_run) has the point's whole arithmetic to arrive in.
struct LanesLogRun { double P, L; int E; };  // the product is (P + L) 2^E
template <bool IMG32, bool UNIT, typename Under>
__device__ __forceinline__ void lanes_sums(int k, const ProblemDesc &pd, const PoseLite<double> &ps_, double x, double y, double z,
                                           const LanesStage<typename ImgOf<double, IMG32>::type> &st, bool pair,
                                           double (&acc)[28], double &cost, double &held, LanesLogRun &run, Under under) {
  typedef double T;
  PoseLite<T> ps = ps_;
  if constexpr (UNIT) ps.unit_q = 1;
  const T loss_a = Uni<T>::loss_a(pd);
  unsigned long long bad = st.bad;
  Proj<T> pr;
  pr.cx_ = st.cx_; pr.cy_ = st.cy_; pr.cz_ = st.cz_; pr.iz = st.iz; pr.fu = st.fu; pr.fv = st.fv;
  pr.bx = st.cx_ + ps.t[0]; pr.by = st.cy_ + ps.t[1];
  pr.fxz = Uni<T>::fx(pd) * st.iz; pr.fyz = Uni<T>::fy(pd) * st.iz;
  if (lanes_any(bad)) {  // (the rest of fused_chunk's fix-up; the sample was moved when the rows were asked for)
    asm volatile("" ::: "memory");  // (keeps the uniform branch a branch, as in jacobian_row: no masked moves on the common path)
    if (lanes_mine(bad)) {
      pr.iz = T(1);
      pr.bx = T(0); pr.by = T(0);
      pr.fxz = T(0); pr.fyz = T(0);
    }
  }
  under();
  T f, Fu, Fv;
  bicubic<T>(pr.fu, pr.fv, [&](int l) { return lanes_widen(st.row[l]); }, f, Fu, Fv);
  T J[6];
  jacobian_row<T>(pd, ps, pr, x, y, z, Fu, Fv, J);
  // (The row is asked for HERE: left alone, the compiler moves the gradient and the Jacobian down behind the loss, next to the
  // sums that use them, and the sixteen widened taps stay alive across the loss's branches -- thirty-two registers at the
  // loop's peak, where the row takes twelve.  That difference is what lets the pose stay in registers: lanes_run.)
  if constexpr (UNIT) asm volatile("" ::"v"(J[0]), "v"(J[1]), "v"(J[2]), "v"(J[3]), "v"(J[4]), "v"(J[5]));
  T rho, w;
  if (UNIT && pair) {
    // loss_point's Cauchy statements; its two selects for a lane without a valid point go behind the uniform branch
    const T xs = (f * f) * Uni<T>::loss_inv_b(pd);
    rho = xs + T(1);
    w = t_rcp<T>(rho);
    if (lanes_any(bad)) {
      asm volatile("" ::: "memory");  // (keeps the uniform branch a branch, as in jacobian_row)
      if (lanes_mine(bad)) { w = T(0); rho = T(1); }
    }
    // the factor into the lane's running product (ea_pair_log.h); the renormalisation is rare: uniform test first
    T p = run.P * rho;
    const bool high = pl_run_high<LogOps>(p);
    if (__any(high)) {
      asm volatile("" ::: "memory");
      if (high) p = pl_run_renorm<LogOps>(run.P, run.L, run.E, rho);
    }
    pl_run_take(run.P, run.L, rho, p);
  } else {
    if constexpr (UNIT) asm volatile("" ::: "memory");  // (kept a branch: nothing of `cost` and `held` on the unit Cauchy path)
    loss_point<T, 2, false>(pair, pd.loss_kind, loss_a, Uni<T>::loss_inv_b(pd), f * f, !lanes_mine(bad), T(1), rho, w);
    cost_point<T, 2>(k, pair, loss_a, rho, cost, held);
  }
  const T wr = w * f;
  int s = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    const T wJa = w * J[a];
#pragma unroll
    for (int b = a; b < 6; ++b) { acc[s] = t_fma<T>(wJa, J[b], acc[s]); ++s; }
    acc[kAccJtr + a] = t_fma<T>(J[a], wr, acc[kAccJtr + a]);
  }
}

// A wavefront's sub-run of n_sub points at px / py / pz, two per iteration: both points are projected and their eight row
// loads issued before the first is summed -- one trip to memory per pair, which the SIMD's other wavefront covers.  (Staging
// the NEXT pair's rows under the sums as well was tried: with 56 registers of sums it does not fit 256 registers without
// scratch.)  The running product of lanes_sums starts at 1 in front of the loop and becomes the cost, (a^2 / 2) log, behind it.
//
// How the loop is pipelined (UNIT): nothing in it waits for anything but the pair's own eight row loads.
//   R, t         stay in the lane's registers from the first point to the last: no read, no wait.  (They used to come out of
//                an LDS copy per pair, and t_x, t_y once more per point, each read used at once; with the Jacobian row pinned
//                in front of the loss -- lanes_sums -- the loop has the twenty-four registers to spare.)
//   coordinates  wave-uniform, scalar loads (ea_lanes_stream.h says which indices in which iteration): ONE pair ahead, one
//                16-byte load per array, straight into the scalar registers the next iteration's projections read -- x, y, z
//                are dead once both points are projected (the unit Jacobian works on R a), so nothing is copied at the
//                back-edge.  They are issued behind the second point's bx, by; the first instruction that needs them, and the
//                only wait they meet, is the next iteration's first projection: the second point's taps, Jacobian, loss and
//                27 sums later, some 170 vector instructions.  The end of a sub-run takes clamped 8-byte loads.
// The general-quaternion form reads x, y, z in its Jacobian and copies the pair it loaded ahead.
template <bool BUF, bool IMG32, bool UNIT>
__device__ __forceinline__ void lanes_run(const ProblemDesc &pd, const PoseLite<double> &ps, CPtr<double> px, CPtr<double> py,
                                          CPtr<double> pz, int n_sub, bool pair, double (&acc)[28], int &n_bad) {
  typedef double T;
  typedef typename ImgOf<T, IMG32>::type IT;
  typedef T T2 __attribute__((ext_vector_type(2), aligned(8)));  // two adjacent points of an array: one 16-byte scalar load
  if (n_sub <= 0) return;
  // (wave-uniform, and said so: left in a vector register, the addresses of the scalar loads are formed by vector
  // instructions and read back lane 0 by lane 0)
  n_sub = __builtin_amdgcn_readfirstlane(n_sub);
  const int iters = lanes_stream_iters(n_sub);
  LanesLogRun run = {T(1), T(0), 0};
  // slot k of the stream (ea_lanes_stream.h) into the pair (x, y, z)
  const auto load_pair = [&](int k, T (&x)[2], T (&y)[2], T (&z)[2]) {
    const LanesStreamLoad ld = lanes_stream_load(k, n_sub);
    if (ld.wide) {
      const T2 vx = *(const CPtr<T2>)(px + ld.i0), vy = *(const CPtr<T2>)(py + ld.i0), vz = *(const CPtr<T2>)(pz + ld.i0);
      x[0] = vx.x; x[1] = vx.y; y[0] = vy.x; y[1] = vy.y; z[0] = vz.x; z[1] = vz.y;
    } else {  // (the end of the sub-run)
      asm volatile("" ::: "memory");
      x[0] = px[ld.i0]; x[1] = px[ld.i1]; y[0] = py[ld.i0]; y[1] = py[ld.i1]; z[0] = pz[ld.i0]; z[1] = pz[ld.i1];
    }
  };
  T X[2], Y[2], Z[2];  // this iteration's pair; UNIT: loaded by the iteration in front of it
  load_pair(-1, X, Y, Z);
#pragma nounroll
  for (int k = 0; k < iters; ++k) {
    T held, cost;  // (set and read behind the kept branch of every loss but the unit Cauchy one)
    LanesStage<IT> A, B;
    lanes_stage<BUF, IMG32>(pd, ps, X[0], Y[0], Z[0], true, A, n_bad);
    // (both points' rows are under way before the first is summed; the rare general-quaternion form, which reads 27 more
    // words per lane and point, takes them one after the other)
    if constexpr (UNIT) {
      lanes_stage<BUF, IMG32>(pd, ps, X[1], Y[1], Z[1], 2 * k + 1 < n_sub, B, n_bad);
      lanes_sums<IMG32, true>(0, pd, ps, T(0), T(0), T(0), A, pair, acc, cost, held, run, []() {});
      lanes_sums<IMG32, true>(1, pd, ps, T(0), T(0), T(0), B, pair, acc, cost, held, run, [&]() { load_pair(k, X, Y, Z); });
    } else {
      T NX[2], NY[2], NZ[2];
      load_pair(k, NX, NY, NZ);
      lanes_sums<IMG32, false>(0, pd, ps, X[0], Y[0], Z[0], A, pair, acc, cost, held, run, []() {});
      lanes_stage<BUF, IMG32>(pd, ps, X[1], Y[1], Z[1], 2 * k + 1 < n_sub, B, n_bad);
      lanes_sums<IMG32, false>(1, pd, ps, X[1], Y[1], Z[1], B, pair, acc, cost, held, run, []() {});
#pragma unroll
      for (int j = 0; j < 2; ++j) { X[j] = NX[j]; Y[j] = NY[j]; Z[j] = NZ[j]; }
    }
    if (!(UNIT && pair)) {
      asm volatile("" ::: "memory");  // (kept a branch, as the fix-ups are)
      acc[kAccCost] += cost;
    }
  }
  if (UNIT && pair) acc[kAccCost] = (T(0.5) * (Uni<T>::loss_a(pd) * Uni<T>::loss_a(pd))) * pl_run_log<LogOps>(run.P, run.L, run.E);
}

// ---- the fold inside the launch: two levels of tickets (ea_poses_map.h, "the rows of the lanes path") --------------------
// An arrival, by the whole workgroup behind its plain stores: every wavefront waits for its own stores, the barrier collects
// them, thread 0 releases at agent scope, waits again (the fence's own wait is not relied on) and takes a ticket with a
// relaxed add; the thread whose ticket completes `target` acquires at agent scope.  Whether the workgroup is that last
// arrival comes back to everybody through `s_word`, a word of the LDS array the kernel already has (the barrier in front
// of its store has every earlier reader of that array behind it).  Nobody waits for anybody: a workgroup that is not the
// last one leaves.
__device__ __forceinline__ bool lanes_ticket(unsigned int *counter, unsigned int target, volatile int *s_word) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned int prev = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = prev + 1u == target;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    *s_word = last;
  }
  __syncthreads();
  return *s_word != 0;
}
// n blocks of kPosesLanesBlock doubles, `stride` doubles apart, summed in block order: lane = pose, the 29 slots dealt over
// the four wavefronts (slot = wave + 4 j), four blocks' loads in flight per slot.  v[j] = sum of slot wave + 4 j.
constexpr int kLanesFoldSlots = (kLanesVals + kLanesWaves - 1) / kLanesWaves;
__device__ __forceinline__ void lanes_fold_blocks(const double *src, size_t stride, int n, int wave, int lane, double (&v)[kLanesFoldSlots]) {
#pragma unroll
  for (int j = 0; j < kLanesFoldSlots; ++j) v[j] = 0.0;
  const double *p = src + lane;
  int r = 0;
  for (; r + 4 <= n; r += 4) {
    double x[4][kLanesFoldSlots];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int j = 0; j < kLanesFoldSlots; ++j) {
        const int slot = wave + kLanesWaves * j;
        x[u][j] = slot < kLanesVals ? p[(size_t)(r + u) * stride + (size_t)slot * kPosesLanes] : 0.0;
      }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int j = 0; j < kLanesFoldSlots; ++j) v[j] += x[u][j];
  }
  for (; r < n; ++r) {
    double x[kLanesFoldSlots];
#pragma unroll
    for (int j = 0; j < kLanesFoldSlots; ++j) {
      const int slot = wave + kLanesWaves * j;
      x[j] = slot < kLanesVals ? p[(size_t)r * stride + (size_t)slot * kPosesLanes] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < kLanesFoldSlots; ++j) v[j] += x[j];
  }
}
// What an item does behind the store of its row.  s_lds: the kernel's LDS array, free by now (>= kAccSlots x 65 doubles).
// group: of the launch; row0 / nrows: the problem's rows; chunk: the item's row in the problem; live: poses of the group.
__device__ __forceinline__ void lanes_tickets(const PosesTickets &tk, const double *rows_base, int rows, int group, int problem,
                                              int row0, int nrows, int chunk, int pose0, int live, int groups, double *s_lds) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  volatile int *s_word = reinterpret_cast<volatile int *>(s_lds);
  const int count = tk.count, run = poses_lanes_run(chunk), slot1 = poses_lanes_run_slot(row0, problem, run);
  // level 1: the last row of the run to arrive sums the run
  if (!lanes_ticket(tk.counters + poses_lanes_counter1(group, slot1, rows, count), (unsigned)poses_lanes_run_rows(nrows, run), s_word)) return;
  double v[kLanesFoldSlots];
  lanes_fold_blocks(rows_base + poses_lanes_row_off(group, row0 + run * kPosesRun, rows), (size_t)kPosesLanesBlock,
                    poses_lanes_run_rows(nrows, run), wave, lane, v);
  double *part = tk.partials + poses_lanes_partial_off(group, slot1, rows, count);
#pragma unroll
  for (int j = 0; j < kLanesFoldSlots; ++j) {
    const int slot = wave + kLanesWaves * j;
    if (slot < kLanesVals) part[(size_t)slot * kPosesLanes + lane] = v[j];
  }
  // level 2: the last run of the problem to arrive sums the run partials and delivers the group's results
  if (!lanes_ticket(tk.counters + poses_lanes_counter2(groups, group, problem, rows, count), (unsigned)poses_lanes_runs(nrows), s_word)) return;
  lanes_fold_blocks(tk.partials + poses_lanes_partial_off(group, poses_lanes_run_slot(row0, problem, 0), rows, count),
                    (size_t)kPosesLanesBlock, poses_lanes_runs(nrows), wave, lane, v);
  __syncthreads();  // (everybody has read s_word)
  // through LDS, padded to 65 words per slot: in [slot][pose], out pose by pose -- each pose's 256-byte result in one piece
  static_assert(kLanesFoldSlots * kLanesWaves == kAccSlots, "the wavefronts' slots cover a result exactly");
#pragma unroll
  for (int j = 0; j < kLanesFoldSlots; ++j) {
    const int slot = wave + kLanesWaves * j;
    s_lds[slot * 65 + lane] = slot < kLanesVals ? v[j] : 0.0;  // (slots 29 .. 31 of a result are zero)
  }
  __syncthreads();
  {
    const int s = threadIdx.x & (kAccSlots - 1), p0 = threadIdx.x / kAccSlots;
#pragma unroll
    for (int it = 0; it < kPosesLanes / (64 * kLanesWaves / kAccSlots); ++it) {
      const int p = p0 + it * (64 * kLanesWaves / kAccSlots);
      if (p < live) tk.out[(size_t)(pose0 + p) * (size_t)count + (size_t)problem].acc[s] = s_lds[s * 65 + p];
    }
  }
  // the results lie in pinned host memory: every storing wavefront makes its own visible system-wide, then one thread
  // raises the flag of (group of the call, problem) to the call's sequence number
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence_system();
    __hip_atomic_store(tk.flags + poses_lanes_flag(tk.group0 + group, problem, count), tk.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// (two wavefronts per SIMD: 56 registers of sums, two staged points and the arithmetic of a third do not fit three, and
// left to itself the register allocator goes past 256 into accumulation registers, which halves the occupancy again)
// Rows and fold.  Lane l of wavefront 0 stores its 29 values lane-minor -- rows[group][row][slot][l], one 512-byte line per
// slot -- into the launch's ONE row array; lanes without a pose of the launch, or with an inactive one, store zeros, and an
// item whose 64 lanes are all like that skips the points and stores zeros too: every item of the list arrives.  Behind the
// store the item takes its tickets (lanes_tickets above): runs of kPosesRun = 16 rows -- a run is 256 KB for its last arrival
// to read, a few microseconds, and C2's 98 rows leave 7 partials to the problem's last arrival -- summed in row order, then
// the run partials in run order.  A pose's bits depend on the pose and the problem's row count: not on the lane, the company,
// the split into launches, the item order or who arrived last.
template <bool BUF, bool IMG32>
__global__ __launch_bounds__(64 * kLanesWaves) __attribute__((amdgpu_waves_per_eu(2, 2))) void ea_eval_poses_lanes_kernel(
    int shape, int g, int rows, const ProblemDesc *__restrict__ probs, const PoseState *__restrict__ poses,
    double *rows_out, PosesTickets tk) {
  typedef double T;
  __shared__ __align__(16) double s_sum[kLanesWaves / 2][kLanesVals][64];
  static_assert(sizeof(s_sum) >= sizeof(double) * kAccSlots * 65, "the fold's transposition fits the sums' array");
  const PosesLanesWork w = poses_lanes_work(blockIdx.x, shape, rows, g, 0);
  if (w.kind != 2) return;  // (uniform; not an item of the list)
  const PosesLanesChunk pc = poses_lanes_chunk(w.row, shape, reinterpret_cast<const PosesRow *>(probs) - rows);
  const ProblemDesc pd = probs[pc.term];
  const long long start = (long long)pc.chunk * (kLanesWaves * kLanesSub);
  const int count = (int)max(0ll, min((long long)(kLanesWaves * kLanesSub), (long long)pd.n - start));
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // the lane's pose; lanes past the launch's last pose compute a copy of it and store zeros
  const PoseState *psp = poses + ((size_t)(w.pose0 + min(lane, w.live - 1)) * (size_t)pc.count + (size_t)pc.term);
  PoseLite<T> ps;
  int active;
  load_pose_lite<T>(psp, ps, active);
  const bool on = lane < w.live && active != 0;

  T v[kLanesVals];
#pragma unroll
  for (int i = 0; i < kLanesVals; ++i) v[i] = T(0);
  if (__any(on)) {  // (the same in the workgroup's four wavefronts: they hold the same poses)
    const int first = wave * kLanesSub, n_sub = max(0, min(kLanesSub, count - first));
    const CPtr<T> px = (CPtr<T>)(static_cast<const T *>(pd.x) + start + first);
    const CPtr<T> py = (CPtr<T>)(static_cast<const T *>(pd.y) + start + first);
    const CPtr<T> pz = (CPtr<T>)(static_cast<const T *>(pd.z) + start + first);
    const bool pair = pd.loss_kind == 1;  // one log per two points (loss_point)
    T acc[28];
#pragma unroll
    for (int i = 0; i < 28; ++i) acc[i] = T(0);
    int n_bad = 0;
    if (__all(ps.unit_q != 0)) lanes_run<BUF, IMG32, true>(pd, ps, px, py, pz, n_sub, pair, acc, n_bad);
    else lanes_run<BUF, IMG32, false>(pd, ps, px, py, pz, n_sub, pair, acc, n_bad);

    // (w0 + w1) + (w2 + w3), lane by lane: the odd member of each pair hands its sums over, then the pair sums do the same
#pragma unroll
    for (int i = 0; i < 28; ++i) v[i] = acc[i];
    v[28] = (T)n_bad;
#pragma unroll
    for (int s = 1; s < kLanesWaves; s <<= 1) {
      const int role = wave & (2 * s - 1), buf = wave / (2 * s);
      if (role == s) {
#pragma unroll
        for (int i = 0; i < kLanesVals; ++i) s_sum[buf][i][lane] = v[i];
      }
      __syncthreads();
      if (role == 0) {
#pragma unroll
        for (int i = 0; i < kLanesVals; ++i) v[i] += s_sum[buf][i][lane];
      }
      if (2 * s < kLanesWaves) __syncthreads();  // (read before the next level writes)
    }
  }
  const int group = w.pose0 / kPosesLanes;
  if (wave == 0) {
    double *o = rows_out + poses_lanes_row_off(group, w.row, rows) + lane;
#pragma unroll
    for (int i = 0; i < kLanesVals; ++i) o[(size_t)i * kPosesLanes] = on ? v[i] : 0.0;
  }
  if (!tk.on) return;
  lanes_tickets(tk, rows_out, rows, group, pc.term, w.row - pc.chunk, pd.tile_end - pd.tile_begin, pc.chunk, w.pose0, w.live,
                poses_lanes_groups(g), &s_sum[0][0][0]);
}

// ---- cost-only pose-batched evaluation (ea_batch_cost_resident_poses) ---------------------------------------------------
// What a ranking of candidate poses, a line search or a cost-surface probe asks for: 1/2 sum rho(r^2) and the failed-functor
// count, nothing else.  ea_cost_poses_kernel takes ea_eval_poses_kernel's work items -- the same flat, XCD-dealt list, chunks,
// descriptor / row-table fetch, point loads and pose slots -- and runs per point the projection, the four row loads, the
// VALUE of the Catmull-Rom patch and rho: no derivative weights, no 1x6 row, no JtJ / Jtr products, two sums instead of 28.

// the four tap weights of cr_weights alone (the same expressions: the sample is bicubic's f to the bit)
template <typename T>
__device__ __forceinline__ void cr_weights_value(T x, T w[4]) {
  const T x2 = x * x;
  const T c15 = s_const(T(1.5));
  w[0] = x * t_fma<T>(x, t_fma<T>(T(-0.5), x, T(1)), T(-0.5));
  w[1] = t_fma<T>(x2, t_fma<T>(c15, x, T(-2.5)), T(1));
  w[2] = x * t_fma<T>(x, t_fma<T>(-c15, x, T(2)), T(0.5));
  w[3] = x2 * t_fma<T>(T(0.5), x, T(-0.5));
}
// 16 taps -> value: bicubic's f, no Fu / Fv
template <typename T, typename RowFn>
__device__ __forceinline__ T bicubic_value(T fu, T fv, RowFn row) {
  T wu[4], wv[4];
  cr_weights_value<T>(fu, wu);
  cr_weights_value<T>(fv, wv);
  T f = T(0);
#pragma unroll
  for (int l = 0; l < 4; ++l) {
    const Row4<T> r = row(l);
    const T rs = t_fma<T>(wu[3], r.p3, t_fma<T>(wu[2], r.p2, t_fma<T>(wu[1], r.p1, wu[0] * r.p0)));
    f = t_fma<T>(wv[l], rs, f);
  }
  return f;
}

// One value per lane summed over the wavefront without LDS: DPP inside a 16-lane row (L ^ 1, L ^ 2, L ^ 7, L ^ 15), then
// v_permlane16_swap / v_permlane32_swap of two copies -- odd rows of one against even rows of the other, upper half-wave
// against lower -- whose sum is the pairing L ^ 16 (L ^ 32).  Every lane ends with the same total; the order is fixed.
template <int CTRL> __device__ __forceinline__ int lane_xchg(int x) { return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xF, 0xF, true); }
template <int W>
__device__ __forceinline__ void swap_rows_b32(unsigned &a, unsigned &b) {
  if constexpr (W == 32) asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 0" : "+v"(a), "+v"(b));
  else asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 0" : "+v"(a), "+v"(b));
}
template <int W> __device__ __forceinline__ float swap_add(float x) {
  unsigned a = __builtin_bit_cast(unsigned, x), b = a;
  swap_rows_b32<W>(a, b);
  return __builtin_bit_cast(float, a) + __builtin_bit_cast(float, b);
}
template <int W> __device__ __forceinline__ int swap_add(int x) {
  unsigned a = (unsigned)x, b = a;
  swap_rows_b32<W>(a, b);
  return (int)(a + b);
}
template <int W> __device__ __forceinline__ double swap_add(double x) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, x);
  unsigned al = (unsigned)u, ah = (unsigned)(u >> 32), bl = al, bh = ah;
  if constexpr (W == 32)
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %2\n\tv_permlane32_swap_b32 %1, %3\n\ts_nop 0" : "+v"(al), "+v"(ah), "+v"(bl), "+v"(bh));
  else
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %2\n\tv_permlane16_swap_b32 %1, %3\n\ts_nop 0" : "+v"(al), "+v"(ah), "+v"(bl), "+v"(bh));
  return __builtin_bit_cast(double, ((unsigned long long)ah << 32) | al) + __builtin_bit_cast(double, ((unsigned long long)bh << 32) | bl);
}
template <typename V>
__device__ __forceinline__ V wave_sum1(V x) {
  x += lane_xchg<kDppQuadXor1>(x);
  x += lane_xchg<kDppQuadXor2>(x);
  x += lane_xchg<kDppRowHalfMirror>(x);
  x += lane_xchg<kDppRowMirror>(x);
  x = swap_add<16>(x);
  return swap_add<32>(x);
}
// Two values per lane summed over the workgroup: each wavefront's sum (in the value's own type), one LDS slot per wavefront,
// and lane 0 adds the slots in wave order -- the first in fp64.  The totals are lane 0's alone.
template <int NT, typename A, typename B>
__device__ __forceinline__ void workgroup_sum2(A a, B b, double &total_a, B &total_b) {
  __shared__ double s_a[NT / 64];
  __shared__ B s_b[NT / 64];
  const int tid = threadIdx.x;
  const A wa = wave_sum1<A>(a);
  const B wb = wave_sum1<B>(b);
  if ((tid & 63) == 0) { s_a[tid >> 6] = (double)wa; s_b[tid >> 6] = wb; }
  __syncthreads();
  if (tid == 0) {
    double ta = 0.0;
    B tb = 0;
#pragma unroll
    for (int v = 0; v < NT / 64; ++v) { ta += s_a[v]; tb += s_b[v]; }
    total_a = ta; total_b = tb;
  }
}

// one narrow partial per workgroup of the cost-only launches: 16 bytes at pose * rows + row
struct __attribute__((aligned(16))) CostPartial { double cost, failed; };
static_assert(sizeof(CostPartial) == kCostPartialBytes, "ea_launch.h");

// item pc of a cost-only launch into its row; false: nothing to evaluate, nothing stored
template <typename T, int PPT, int NT, bool BUF, bool IMG32>
__device__ __forceinline__ bool cost_item(const void *__restrict__ x0, const void *__restrict__ y0, const void *__restrict__ z0, int n0,
                                          const ProblemDesc *__restrict__ probs, const PoseState *__restrict__ poses,
                                          const PosesChunk &pc, CostPartial *__restrict__ partials) {
  typedef typename ImgOf<T, IMG32>::type IT;
  const int tid = threadIdx.x;
  EA_ITEM_HEAD(false, NT * PPT, pc.chunk, pc.term, pc.slot, false, return false);
  const int pitch = pd.pitch;
  const void *img_base = IMG32 ? pd.dt32 : pd.dt;
  const GPtr<IT> gimg = (GPtr<IT>)(static_cast<const IT *>(img_base) + (size_t)kImagePad * (size_t)pitch + kImagePad);
  const __amdgpu_buffer_rsrc_t rimg =
      make_raw_buffer(img_base, BUF ? (unsigned)pitch * (unsigned)(pd.H + 2 * kImagePad) * (unsigned)sizeof(IT) : 0u);
  const int loss_kind = pd.loss_kind;
  const T loss_a = Uni<T>::loss_a(pd), loss_inv_b = Uni<T>::loss_inv_b(pd);
  // projection; lanes past the end of the chunk and lanes whose functor fails move to a harmless sample and get weight 0
  Proj<T> pr[PPT];
  bool valid[PPT];
  int n_bad = 0;
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    const bool inb = tid + k * NT < count;
    project_point<T>(pd, ps, X[k], Y[k], Z[k], pr[k]);
    valid[k] = inb && pr[k].state == 1;
    n_bad += (inb && pr[k].state == 2) ? 1 : 0;
    if (__any(!valid[k]) && !valid[k]) {  // (uniform test first: the common wavefront has nothing to fix up)
      pr[k].iu = 0; pr[k].iv = 0; pr[k].fu = T(0); pr[k].fv = T(0);
    }
  }
  T acc = T(0), held = T(1);
  const bool pair = loss_kind == 1;  // one log per lane (loss_point)
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    T f;
    if constexpr (BUF) {
      // byte offset of texel (iv - 1, iu - 1) in the padded image; iv, iu >= -2 keeps it non-negative
      const int voff = ((pr[k].iv + (kImagePad - 1)) * pitch + (pr[k].iu + (kImagePad - 1))) * (int)sizeof(IT);
      f = bicubic_value<T>(pr[k].fu, pr[k].fv, [&](int l) { return RowLoad<T, IT>::buf(rimg, voff, l * pitch * (int)sizeof(IT)); });
    } else {
      const GPtr<IT> base = gimg + ((ptrdiff_t)(pr[k].iv - 1) * pitch + (pr[k].iu - 1));
      f = bicubic_value<T>(pr[k].fu, pr[k].fv, [&](int l) { return RowLoad<T, IT>::flat(base + (ptrdiff_t)l * pitch); });
    }
    T rho, wt;
    loss_point<T, PPT, false>(pair, loss_kind, loss_a, loss_inv_b, f * f, valid[k], T(1), rho, wt);
    cost_point<T, PPT>(k, pair, loss_a, rho, acc, held);
  }
  // a wavefront's sum in T, the workgroup's in fp64 through LDS in wave order: fixed by (chunk, lane, wave)
  double c;
  int nb;
  workgroup_sum2<NT>(acc, n_bad, c, nb);
  if (tid == 0) partials[pc.out_row] = CostPartial{c, (double)nb};
  return true;
}

template <typename T, int PPT, int NT, bool BUF, bool IMG32 = false>
__global__ __launch_bounds__(NT) void ea_cost_poses_kernel(
    const void *__restrict__ x0, const void *__restrict__ y0, const void *__restrict__ z0, int n0,
    int shape, int g, int rows,
    const ProblemDesc *__restrict__ probs, const PoseState *__restrict__ poses,
    CostPartial *__restrict__ partials) {
  static_assert(!IMG32 || std::is_same<T, double>::value, "fp32-stored image: fp64 kernels");
  const PosesWork w = poses_work(blockIdx.x, shape, rows, g, 0);
  if (w.kind != 2) return;  // (uniform)
  const PosesChunk pc = poses_chunk(w, shape, rows, reinterpret_cast<const PosesRow *>(probs) - rows);
  if (!cost_item<T, PPT, NT, BUF, IMG32>(x0, y0, z0, n0, probs, poses, pc, partials) && threadIdx.x == 0)
    partials[pc.out_row] = CostPartial{0.0, 0.0};
}

// The fold of a cost-only launch: one 256-lane workgroup per (pose, problem) of the launch sums the pose's narrow partials
// of the problem's rows -- lane l rows l, l + 256, .. in row order, the wavefronts' sums in wave order, all fp64 -- and writes
// {cost, n_invalid} into the cost and invalid slots of the result in pinned host memory, then counts itself in and the last
// arrival raises the pinned flag to the launch's sequence number (poses_fold_one's signal).
template <int NT>
__global__ __launch_bounds__(NT) void ea_cost_fold_kernel(PosesFold f) {
  const int tid = threadIdx.x, r = blockIdx.x;
  int pose, problem;
  poses_rider(r, f.count, &pose, &problem);
  const GroupDesc gd = f.groups[problem];
  const CostPartial *rows = reinterpret_cast<const CostPartial *>(f.rows) + (size_t)pose * f.rows_per_pose;
  double c = 0.0, nb = 0.0;
  for (int i = gd.tile_begin + tid; i < gd.tile_end; i += NT) {
    const CostPartial p = rows[i];
    c += p.cost; nb += p.failed;
  }
  double ct, nt;
  workgroup_sum2<NT>(c, nb, ct, nt);
  if (tid == 0) {
    f.out[r].acc[kAccCost] = ct;
    f.out[r].acc[kAccInvalid] = nt;
    signal_done(f.counter, (unsigned)f.n, f.host_flag, f.seq);
  }
}

// The evaluation of a multi-start solve (ea_batch_solve_starts): ea_eval_poses_kernel's launch -- the same one-dimensional,
// XCD-dealt item list, chunks, per-point code and row index pose * rows + row, so a start's partial rows hold the bits the
// pose-batched evaluation gives for that pose -- over a piece of the LIVE LIST (ea_starts_map.h): item pose g of the launch is
// position off + g of the list, evaluates start live[off + g] at its pose slot start * count + term, and writes the rows
// g * rows + row.  n_live is a word on the device: the host sizes the grid from the last value it has seen, and positions
// from n_live on return at once.  No riders: the step kernel of the pair folds the rows.
template <typename T, int PPT, int MODE, int NT, bool VAR, bool BUF, bool IMG32 = false>
__global__ __launch_bounds__(NT) void ea_eval_starts_kernel(
    const void *__restrict__ x0, const void *__restrict__ y0, const void *__restrict__ z0, int n0,
    int shape, int g, int rows,
    const ProblemDesc *__restrict__ probs, const PoseState *__restrict__ poses,
    double *__restrict__ partials, const int *__restrict__ live, const int *__restrict__ n_live, int off) {
  static_assert((MODE == 0 || MODE == kModeExchange) && !VAR, "plain functor, stencil rows from L2");
  constexpr bool XCHG = MODE == kModeExchange;
  extern __shared__ __align__(16) unsigned char smem[];
  double *s_red = reinterpret_cast<double *>(smem);
  int *s_box = reinterpret_cast<int *>(smem + kRedBytes);
  const PosesWork w = poses_work(blockIdx.x, shape, rows, g, 0);
  if (w.kind != 2) return;  // (uniform)
  if (!starts_position_live(off, w.pose, *n_live)) return;
  const int start_k = live[off + w.pose];
  const PosesChunk pc = starts_chunk(w, start_k, shape, rows, reinterpret_cast<const PosesRow *>(probs) - rows);
  const int tid = threadIdx.x;
  EA_ITEM_HEAD(false, NT * PPT, pc.chunk, pc.term, pc.slot, false, return);
  const double sum = fused_chunk<T, PPT, 0, NT, false, BUF, IMG32, PoseLite<T>, XCHG>(pd, ps, X, Y, Z, count, s_red, s_box, (T *)nullptr, 0,
                                                                                       tid < kAccSlots ? tid : -1);
  store_row_sum<XCHG>(partials, pc.out_row, sum);
}

// SIDE instantiations of the LM kernels.  Problem p's PriorDesc (ea_prior.h; the table sits behind the group table) is
// fetched one 8-byte word per lane beside the state words, before the fold (prior_word), and parked in LDS with them
// (prior_lds) -- its load is not a dependent round trip on the state machine's critical path.  After the barrier lane 0 adds
// the priors to the folded sums in LDS, at the pose they were evaluated at -- st.x before the first evaluation, st.cand
// after -- and the workgroup waits for it.  The state machine then reads s_acc exactly as the prior-free instantiation does:
// its code is the same, so a problem without a prior in a batch with priors takes bit for bit the steps of its own solve.
// Constant tangent coordinates (ea_problem_set_constant_parameters) ride the same instantiations: a batch with a mask on any
// problem has the table (a record without priors adds nothing), and behind the priors lane 0 replaces the held rows and columns
// of the sums by a unit diagonal and the held gradient by zero (lm_mask_system, ea_lm.h; the mask itself travels in
// LMState::held, where lm_init put it).  The state machine runs with MASK = SIDE: x_norm over the non-constant blocks and
// the all-held exit; with nothing held it is the arithmetic of the mask-free code, bit for bit.
constexpr int kPriorWords = (int)(sizeof(PriorDesc) / 8);
__device__ __forceinline__ PriorDesc &prior_lds() {
  __shared__ PriorDesc s_prior;  // (only the SIDE instantiations reference it)
  return s_prior;
}
__device__ __forceinline__ double prior_word(const GroupDesc *__restrict__ groups, int nprob, int p, int tid) {
  return tid < kPriorWords ? reinterpret_cast<const double *>(reinterpret_cast<const PriorDesc *>(groups + nprob) + p)[tid] : 0.0;
}
__device__ __forceinline__ void prior_into_lds(const LMState &s_st, double *s_acc, int tid) {
  if (tid == 0) {
    double acc[kAccSlots];
#pragma unroll
    for (int i = 0; i < kAccSlots; ++i) acc[i] = s_acc[i];
    prior_add(prior_lds(), s_st.num_evals == 0 ? s_st.x : s_st.cand, acc);
    lm_mask_system(s_st.held, acc);
#pragma unroll
    for (int i = 0; i < kAccSlots; ++i) s_acc[i] = acc[i];
  }
  __syncthreads();
}

// ---- the trust-region step, once: the pieces ea_lm_step_kernel, ea_lm_step_starts_kernel and ea_lm_iter_kernel are made of
//
// A step folds a problem's partial rows, advances the trust-region state machine and publishes the next pose to evaluate.
// The state machine is scalar fp64 work on lane 0 (pure latency: ~1/3 of an LM iteration), so everything around it is
// arranged to overlap: the state words travel while the partial rows are fetched (sixteen 16-byte loads in flight per lane),
// the host's progress counter is posted before the arithmetic, lane 0 works on a register copy of the state, and the pose's
// float mirrors / the write-back are lane-parallel.  In the order of a step:
//   EA_LM_PIN_OPTIONS          the options out of the kernel argument segment, in one batch of scalar loads behind one wait
//   lm_state_word, prior_word  one 8-byte word of the state (and of the prior record) per lane, issued IN FRONT of the fold
//   (the fold: the caller's -- reduce_tiles<., 8> over the problem's range, or <., 4> over pose * rows + range for a start)
//   lm_step_park               the words into LDS, the barrier, the priors and the mask into the folded sums (prior_into_lds)
//   EA_LM_STEP_LANE0           lane 0: register copy of state and sums, lm_begin / lm_advance, the candidate pose into LDS
//   lm_step_publish            state words and pose to memory, lane-parallel
//   EA_LM_STEP_DELIVER         a solve that ends: final state and trace rows straight into pinned host memory
// Every piece takes tid and derives nothing from the workgroup's shape.  What orders a kernel against the host or against
// other workgroups (progress words, alive counts, what follows the delivery) stays in the kernel.
// The two pieces that hold objects of their own (the register copy of the state; the row copier and the second LMPending)
// are statement macros: as functions, in every form tried, they moved those objects in front of the kernel's and
// ea_lm_iter_kernel -- 10 000 instructions at 384 VGPRs -- came out 5 .. 50 vector instructions longer in most instantiations
// (profiles/step_tail_listing.md).  As macros the kernels compile to the code they had when each held its own copy.
constexpr int kStateWords = (int)(sizeof(LMState) / 8), kColdWords = (int)(sizeof(LMCold) / 8);
constexpr int kPoseDoubles = 4 + 3 + 9 + 27, kPoseFloats = 9 + 3 + 27;  // q | t | R | G, and Rf | tf | Gf behind them
static_assert(sizeof(LMState) % 8 == 0 && kStateWords <= kLmThreads && kColdWords <= 64, "one 8-byte word per lane (cold: per lane of a wavefront)");
static_assert(offsetof(PoseState, Rf) == kPoseDoubles * 8 && offsetof(PoseState, unit_q) == kPoseDoubles * 8 + kPoseFloats * 4,
              "PoseState layout");

// Everything the kernel argument segment holds is fetched where this stands, in one batch of scalar loads behind one wait:
// left to the compiler, the options were loaded where lane 0 first uses them -- two more cold misses of the argument
// segment on the state machine's critical path, after the fold.
#define EA_LM_PIN_OPTIONS(opt)                                                                                              \
  asm volatile("" : "+s"((opt).max_num_iterations), "+s"((opt).function_tolerance), "+s"((opt).gradient_tolerance),        \
                    "+s"((opt).parameter_tolerance), "+s"((opt).initial_trust_region_radius),                              \
                    "+s"((opt).max_trust_region_radius), "+s"((opt).min_trust_region_radius),                              \
                    "+s"((opt).min_relative_decrease), "+s"((opt).min_lm_diagonal), "+s"((opt).max_lm_diagonal),           \
                    "+s"((opt).max_num_consecutive_invalid_steps), "+s"((opt).jacobi_scaling), "+s"((opt).strategy))

// The words of a step that travel beside the partial rows: lane tid's word of the state (and prior_word above), loaded by
// the kernel in front of its fold, then parked in LDS behind it -- the barrier, and the priors and the mask into the sums.
__device__ __forceinline__ double lm_state_word(const LMState *st, int tid) {
  return tid < kStateWords ? reinterpret_cast<const double *>(st)[tid] : 0.0;
}
template <bool SIDE>
__device__ __forceinline__ void lm_step_park(double state_word, double pw, LMState &s_st, double *s_acc, int tid) {
  if (tid < kStateWords) reinterpret_cast<double *>(&s_st)[tid] = state_word;
  if constexpr (SIDE) {
    if (tid < kPriorWords) reinterpret_cast<double *>(&prior_lds())[tid] = pw;
  }
  __syncthreads();
  if constexpr (SIDE) prior_into_lds(s_st, s_acc, tid);
}

// Lane 0 of a step (inside the caller's `if`; STRAT and SIDE are the kernel's): the state machine on st, a member-by-member
// register copy of the state the caller declares, and on acc, a copy of the folded sums; then the candidate pose into
// *s_ps_.  cold_ is the system at x the state machine reads and updates (global memory, or a wavefront's LDS copy), tr_
// takes the rows of invalid steps (lm_trace) and may be null, STAMP_ is a statement between the state machine and the pose
// (the diagnostic build's clock).  The full form (LITE_ = false) leaves the state in s_st_ and the number of the pending
// trace row in s_trace_it_; acc_ and pend_ are the caller's, lm_flush and EA_LM_STEP_DELIVER take them.  LITE_ (an
// evaluating wavefront of ea_lm_iter_kernel): the pose and nothing else.
#define EA_LM_STEP_LANE0(LITE_, st_, s_st_, s_acc_, cold_, tr_, opt_, s_ps_, s_trace_it_, acc_, pend_, STAMP_)              \
  do {                                                                                                                      \
    lm_copy_state(&(st_), &(s_st_));                                                                                        \
    _Pragma("unroll") for (int i = 0; i < kAccSlots; ++i) (acc_)[i] = (s_acc_)[i];                                          \
    if (EA_UNLIKELY((st_).num_evals == 0)) lm_begin<STRAT, LITE_, SIDE>(&(st_), cold_, tr_, &(opt_), acc_, &(pend_));       \
    else lm_advance<STRAT, LITE_, SIDE>(&(st_), cold_, tr_, &(opt_), acc_, &(pend_));                                       \
    STAMP_;                                                                                                                 \
    make_pose_core((st_).cand, (st_).rot_transposed, (st_).running, s_ps_, /*zero_unused_G=*/false);                        \
    if constexpr (!(LITE_)) {                                                                                               \
      lm_copy_state(&(s_st_), &(st_));                                                                                      \
      s_trace_it_ = (pend_).trace_it;                                                                                       \
    }                                                                                                                       \
  } while (0)

// State and pose of a step to memory, all lanes: the state one 8-byte word per lane; of the pose the doubles by lanes 64..,
// the float mirrors (Rf | tf | Gf of R | t | G) converted by lanes 128.., the flags by lane 192.  G is never read when
// unit_q is set; those lanes publish zeros.
__device__ __forceinline__ void lm_step_publish(const LMState &s_st, const PoseState &s_ps, LMState *st_dst, PoseState *pose_dst, int tid) {
  if (tid < kStateWords) reinterpret_cast<double *>(st_dst)[tid] = reinterpret_cast<const double *>(&s_st)[tid];
  const double *pd_src = reinterpret_cast<const double *>(&s_ps);
  const int a = tid - 64, f = tid - 128;
  const bool skip_g = s_ps.unit_q != 0;
  if (a >= 0 && a < kPoseDoubles) reinterpret_cast<double *>(pose_dst)[a] = (skip_g && a >= 16) ? 0.0 : pd_src[a];
  if (f >= 0 && f < kPoseFloats) {
    const double v = f < 9 ? s_ps.R[f] : (f < 12 ? s_ps.t[f - 9] : (skip_g ? 0.0 : s_ps.G[f - 12]));
    (&pose_dst->Rf[0])[f] = (float)v;
  }
  if (tid == 192) { pose_dst->unit_q = s_ps.unit_q; pose_dst->active = s_ps.active; }
}

// The solve of a problem ends with this launch (the caller's uniform `if (!s_st.running)`): the result goes straight into
// pinned host memory -- final state and the trace rows written so far -- so the host returns without a device-to-host copy
// or a stream synchronisation behind launches that were queued ahead and now have nothing to do.  The caller lowers the flag
// the host polls behind this.  WANTED_ / ROWS_WANTED_ are the caller's (uniform) conditions: the pair and fused forms
// deliver when they were given host_states, a multi-start solve always delivers the state and the rows only with summaries;
// a literal `true` costs nothing.  tr_ / host_tr_: the problem's trace on the device and in host memory; pend_ / acc_ /
// cold_: as lm_flush took them (the system is not stored a second time).  Two arms: usually rows < last come from earlier
// launches, one lane each, and lane 0 holds the last one; when this very launch wrote rows through lm_trace (invalid steps),
// or the solve ran past the trace's end, lane 0 wrote them and lane 0 copies them all.
#define EA_LM_STEP_DELIVER(WANTED_, ROWS_WANTED_, s_st_, trace_it_, pend_, acc_, cold_, tr_, host_st_, host_tr_, tid_)      \
  do {                                                                                                                      \
    if (WANTED_) {                                                                                                          \
      if ((tid_) < kStateWords)                                                                                             \
        reinterpret_cast<double *>(host_st_)[tid_] = reinterpret_cast<const double *>(&(s_st_))[tid_];                      \
      if (ROWS_WANTED_) {                                                                                                   \
        const int last = min((s_st_).iteration, kTrace - 1); /* rows 0 .. last exist */                                     \
        auto copy_row = [&](int r) {                                                                                        \
          const LMTrace &src = *(tr_);                                                                                      \
          LMTrace &dst = *(host_tr_);                                                                                       \
          dst.it_cost[r] = src.it_cost[r];                                                                                  \
          dst.it_cost_change[r] = src.it_cost_change[r];                                                                    \
          dst.it_gradient_max_norm[r] = src.it_gradient_max_norm[r];                                                        \
          dst.it_step_norm[r] = src.it_step_norm[r];                                                                        \
          dst.it_relative_decrease[r] = src.it_relative_decrease[r];                                                        \
          dst.it_radius[r] = src.it_radius[r];                                                                              \
          dst.it_successful[r] = src.it_successful[r];                                                                      \
        };                                                                                                                  \
        if ((trace_it_) == last) {                                                                                          \
          if ((tid_) < last) copy_row(tid_);                                                                                \
          if ((tid_) == 0) {                                                                                                \
            LMPending h = (pend_);                                                                                          \
            h.store_system = 0;                                                                                             \
            lm_flush(&h, cold_, host_tr_, acc_);                                                                            \
          }                                                                                                                 \
        } else if ((tid_) == 0) {                                                                                           \
          __threadfence();                                                                                                  \
          for (int r = 0; r <= last; ++r) copy_row(r);                                                                      \
        }                                                                                                                   \
      }                                                                                                                     \
      __threadfence_system();                                                                                               \
    }                                                                                                                       \
  } while (0)

// LM step, the (evaluate, step) pair form: one workgroup per problem (the pieces above).
// SIDE: the problems' NormalPriors are added to the folded sums before the state machine reads them (prior_into_lds).  The
// prior table sits right behind the group table (one PriorDesc per problem: batch_build lays them out so), so no argument is
// added: the SIDE = false instantiations are the code this kernel was before priors existed.
template <int STRAT, bool SIDE>
__global__ __launch_bounds__(kLmThreads) void ea_lm_step_kernel(
    const GroupDesc *__restrict__ groups, const double *__restrict__ partials,
    PoseState *__restrict__ poses, LMState *__restrict__ states, LMCold *__restrict__ cold,
    LMTrace *__restrict__ traces, LMOptions opt_arg,
    int *__restrict__ progress /* pinned host: [running x n | evals x n] */,
    LMState *__restrict__ host_states, LMTrace *__restrict__ host_traces /* pinned host, nullable: final delivery */,
    GroupDesc first /* = groups[0], by value: problem 0's row range needs no dependent load */,
    int post_done /* also post "this step is complete" (progress[2 n + p]): the point-sharded solve's look-ahead rule */) {
  __shared__ __align__(16) double s_part[reduce_tiles_lds<kLmThreads>()];
  __shared__ double s_acc[kAccSlots];
  __shared__ LMState s_st;
  __shared__ PoseState s_ps;
  __shared__ int s_trace_it;
  const int p = blockIdx.x, tid = threadIdx.x;
#ifdef EA_STAMPS
  const int ev_ = states[p].num_evals;
#endif
  EA_LM_STAMP(0, ev_);
#ifdef EA_STAMPS
  if (threadIdx.x == 0 && blockIdx.x == 0) g_lm_probe_row = ev_ & 63;
#endif
  LMOptions opt = opt_arg;
  EA_LM_PIN_OPTIONS(opt);
  GroupDesc gd = first;
  if (p != 0) gd = groups[p];  // (uniform)
  const int running = states[p].running;
  const int evals_before = states[p].num_evals;  // (a register copy: the LDS copy is rewritten by lane 0 below)
  const double state_word = lm_state_word(states + p, tid);
  double pw = 0.0;
  if constexpr (SIDE) pw = prior_word(groups, gridDim.x, p, tid);
  EA_LM_STAMP(1, ev_);
  // The rows are fetched WITHOUT waiting for the running flag: the flag's round trip (0.5 us of the 2.5 us this kernel spends
  // before its first arithmetic, in-kernel stamps) then travels beside the rows' instead of in front of it.  A finished
  // problem folds rows nobody reads and leaves below.
  reduce_tiles<kLmThreads, 8>(partials, gd.tile_begin, gd.tile_end, s_part, s_acc);
  if (!running) return;  // uniform
  lm_step_park<SIDE>(state_word, pw, s_st, s_acc, tid);
  EA_LM_STAMP(2, ev_);
  // the host only uses this counter to decide how far ahead to enqueue: posted by another wavefront before the
  // arithmetic, so the PCIe write is neither the last thing the kernel waits for nor in lane 0's memory counter
  if (tid == 64)
    __hip_atomic_store(progress + gridDim.x + p, evals_before + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  LMPending pend;
  double acc[kAccSlots];
  if (tid == 0) {
    LMState st;
    EA_LM_STEP_LANE0(false, st, s_st, s_acc, cold + p, traces + p, opt, &s_ps, s_trace_it, acc, pend, EA_LM_STAMP(3, ev_));
    EA_LM_STAMP(4, ev_);
  }
  __syncthreads();
  lm_step_publish(s_st, s_ps, states + p, poses + p, tid);
  if (tid == 0) lm_flush(&pend, cold + p, traces + p, acc);
  if (!s_st.running) {  // uniform: the solve of this problem ends with this launch
    EA_LM_STEP_DELIVER(host_states, true, s_st, s_trace_it, pend, acc, cold + p, traces + p, host_states + p, host_traces + p, tid);
    __syncthreads();  // only behind every lane's delivery does the flag the host polls go down
    if (tid == 0) __hip_atomic_store(progress + p, 0, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  // behind the flag (same lane, release order): a host that has seen "step k complete" sees the flag as step k left it
  if (post_done && tid == 0)
    __hip_atomic_store(progress + 2 * gridDim.x + p, evals_before + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
#ifdef EA_STAMPS
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
  EA_LM_STAMP(5, ev_);
}

// ---- K trust-region runs per problem in lock-step (ea_batch_solve_starts) ------------------------------------------------
//
// The step of one (live position, problem) of a multi-start solve, one 256-lane workgroup each: the pieces of the step
// (above) on the slot live[off + pose] * count + problem.  The rows of the start are folded with reduce_tiles<256, 4> over
// pose * rows + the problem's range -- poses_fold_one's order, so the sums a start steps on are what ea_batch_eval_poses
// folds for that pose, wherever in the list the start sits.  The candidate pose goes into the start's own slot (active = 0
// once its solve has ended); a start that ends always delivers its final state, its trace rows when the call wants
// summaries, and takes itself off its start's count of running problems (alive).
// Nobody waits for another workgroup: what a launch reads of the list, no launch of the same iteration writes (the list and
// its length are ping-ponged by the iteration's parity), and the kernel boundary is the only ordering.
template <int STRAT, bool SIDE>
__device__ __forceinline__ void starts_step_one(const StartsStep &a, const LMOptions &opt, int pose, int problem, int start_k) {
  __shared__ __align__(16) double s_part[reduce_tiles_lds<kLmThreads>()];
  __shared__ double s_acc[kAccSlots];
  __shared__ LMState s_st;
  __shared__ PoseState s_ps;
  __shared__ int s_trace_it;
  const int tid = threadIdx.x;
  const int p = start_k * a.count + problem;
  const GroupDesc gd = a.groups[problem];
  const int running = a.states[p].running;
  const double state_word = lm_state_word(a.states + p, tid);
  double pw = 0.0;
  if constexpr (SIDE) pw = prior_word(a.side, a.count, problem, tid);
  const int base = pose * a.rows_per_pose;
  reduce_tiles<kLmThreads, 4>(a.rows, base + gd.tile_begin, base + gd.tile_end, s_part, s_acc);
  if (!running) return;  // uniform: this problem of the start has ended, a sibling keeps the start in the list
  lm_step_park<SIDE>(state_word, pw, s_st, s_acc, tid);
  LMTrace *const tr = a.traces ? a.traces + p : nullptr;
  LMTrace *const host_tr = a.host_traces ? a.host_traces + p : nullptr;
  LMPending pend;
  double acc[kAccSlots];
  if (tid == 0) {
    LMState st;
    EA_LM_STEP_LANE0(false, st, s_st, s_acc, a.cold + p, tr, opt, &s_ps, s_trace_it, acc, pend, (void)0);
  }
  __syncthreads();
  lm_step_publish(s_st, s_ps, a.states + p, a.poses + p, tid);
  if (tid == 0) lm_flush(&pend, a.cold + p, tr, acc);
  if (!s_st.running) {  // uniform: this solve ends with this launch
    EA_LM_STEP_DELIVER(true, host_tr, s_st, s_trace_it, pend, acc, a.cold + p, tr, a.host_states + p, host_tr, tid);
    if (tid == 0) __hip_atomic_fetch_add(a.alive + start_k, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// One workgroup per (pose of the piece, problem).  In the iteration's LAST step launch every workgroup -- with or without
// work -- counts itself in on an agent-scope counter once its stores are out; the last arrival re-arms the counter, rebuilds
// the live list in order (a start stays while any of its problems runs: alive[start] > 0), writes the new length and posts
// {tag, iterations complete, n_live} to the one pinned word the host polls, with release order.
template <int STRAT, bool SIDE>
__global__ __launch_bounds__(kLmThreads) void ea_lm_step_starts_kernel(StartsStep a, LMOptions opt_arg) {
  __shared__ int s_is_last;
  __shared__ unsigned long long s_masks[4];
  LMOptions opt = opt_arg;
  EA_LM_PIN_OPTIONS(opt);
  const int tid = threadIdx.x;
  const int n_live = *a.n_in;
  int pose, problem;
  starts_step_item(blockIdx.x, a.count, &pose, &problem);
  if (starts_position_live(a.off, pose, n_live))  // (uniform)
    starts_step_one<STRAT, SIDE>(a, opt, pose, problem, a.live_in[a.off + pose]);
  if (!a.last) return;  // (uniform)
  __syncthreads();      // every lane's stores are issued (and fenced where the host reads them) before lane 0 counts in
  if (tid == 0) {
    __threadfence_system();
    const unsigned int prev = __hip_atomic_fetch_add(a.counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    s_is_last = prev == gridDim.x - 1;
  }
  __syncthreads();
  if (!s_is_last) return;  // (uniform)
  int kept = 0;
  for (int first = 0; first < n_live; first += kLmThreads) {  // (uniform bounds)
    const int i = first + tid;
    int start_k = 0;
    bool keep = false;
    if (i < n_live) {
      start_k = a.live_in[i];
      keep = __hip_atomic_load(a.alive + start_k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > 0;
    }
    const unsigned long long m = __ballot(keep);
    if ((tid & 63) == 0) s_masks[tid >> 6] = m;
    __syncthreads();
    uint64_t masks[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) masks[k] = s_masks[k];
    if (keep) a.live_out[starts_compact_slot(masks, tid >> 6, tid & 63, kept)] = start_k;
    kept += starts_compact_kept(masks);
    __syncthreads();
  }
  if (tid == 0) {
    *a.n_out = kept;
    __hip_atomic_store(a.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence_system();
    __hip_atomic_store(a.host_word, (unsigned long long)starts_word(a.tag, a.iteration, kept), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// ---- one launch per LM iteration ----------------------------------------------------------------------------------------
//
// ea_solve's loop as (evaluate, step) pairs pays two kernel boundaries per iteration and, in between, the publication of the
// candidate pose through memory: evaluation kernel ends -> step kernel starts cold on one CU, folds, runs the state machine,
// stores pose and state, ends -> evaluation kernel starts cold, fetches descriptor and pose, ...  For ONE small problem the
// evaluation is at most one workgroup per CU, and every CU but one idles through the step.  Here every workgroup of the
// evaluation runs the step itself: it folds the previous launch's partial rows (the same reduce_tiles in the same order),
// runs the state machine on its lane 0 -- identical instructions on identical inputs, so every workgroup arrives at the same
// candidate pose without talking to the others -- and evaluates its own points at that pose straight away, its point loads
// having travelled beside the fold.  One kernel boundary per iteration instead of two, no pose round trip through memory, and
// the cold start of the evaluation (descriptor, points) hidden behind the fold.  Nothing is handed from one workgroup to
// another inside a launch; what a launch reads (state, cold system, rows) it never writes: those three are ping-ponged
// between two buffers by the parity of the launch.
//
// One more workgroup than chunks: the one past the last chunk has no points and is the WRITER -- state, cold system, trace row,
// the pose (for whoever evaluates at it afterwards), the host's progress words and, when the solve ends, the final delivery
// into pinned host memory, by the pieces ea_lm_step_kernel uses.  Its stores do not sit in any evaluator's memory counter.
// A finished problem is recognised by every later launch from poses[p].active == 0 (written once, by the writer of the
// launch in which the state machine stopped; in that launch every workgroup finds out by itself).
// The cold system (JtJ, Jtr at x for the step after a rejected one; the dogleg's vectors) is read into LDS, one copy per
// wavefront, and the state machine works on that copy; the writer stores its copy for the next launch.
// One plain residual family per problem, 256-thread workgroups, stencil rows from L2; the host only takes this path when the
// whole grid is resident at once (<= 256 workgroups), see solve_start.
// SIDE: as in ea_lm_step_kernel (the prior table behind `groups`): the prior enters the folded sums in LDS once per
// workgroup, before the writer's and every evaluating wavefront's state machine read them, so they stay in lockstep.
template <typename T, int PPT, bool BUF, bool IMG32, int STRAT, bool SIDE>
__global__ __launch_bounds__(kLmThreads) void ea_lm_iter_kernel(
    // the 14 preloaded dwords: what problem 0's point loads and ROW loads need -- the fold is the head of every workgroup's
    // dependent chain, and its loads must not wait for a scalar load of the argument segment (tile0_* = problem 0's row range)
    const void *__restrict__ x0, const void *__restrict__ y0, const void *__restrict__ z0, int n0,
    int shape, int chunks_per_xcd, const double *__restrict__ rows_in, int tile0_begin, int tile0_end,
    const ProblemDesc *__restrict__ probs, PoseState *__restrict__ poses,
    double *__restrict__ rows_out, const GroupDesc *__restrict__ groups,
    const LMState *__restrict__ st_in, LMState *__restrict__ st_out, const LMCold *__restrict__ cold_in,
    LMCold *__restrict__ cold_out, LMTrace *__restrict__ traces, LMOptions opt_arg,
    int *__restrict__ progress /* pinned host: [running x n | evals x n | steps complete x n] */,
    LMState *__restrict__ host_states, LMTrace *__restrict__ host_traces,
    int post_done /* the writer also posts "this step is complete" (progress[2 n + p]): the point-sharded solve's look-ahead rule */) {
  constexpr int NT = kLmThreads;
  __shared__ __align__(16) double s_part[reduce_tiles_lds<NT>()];
  __shared__ double s_acc[kAccSlots];
  __shared__ LMState s_st;
  __shared__ PoseState s_pose[NT / 64];  // one per wavefront (the writer uses the first)
  __shared__ LMCold s_cold[NT / 64];
  __shared__ int s_trace_it, s_store_system;
  extern __shared__ __align__(16) unsigned char smem[];
  double *s_red = reinterpret_cast<double *>(smem);
  int *s_box = reinterpret_cast<int *>(smem + kRedBytes);
  const int chunk = shape & 0xffff, xcd_remap = (shape >> 16) & 1;
  const int p = blockIdx.y, tid = threadIdx.x;
  const int bx = blockIdx.x;
  const int c = xcd_remap ? (bx & 7) * chunks_per_xcd + (bx >> 3) : bx;
  const bool writer = bx == (int)gridDim.x - 1;  // (= the last chunk index in either mapping; the launcher sizes the grid past the data)
  const long long start = (long long)c * chunk;
  LMOptions opt = opt_arg;
  EA_LM_PIN_OPTIONS(opt);
  // problem 0's points go out first (their addresses came with the wave), then everything uniform in one batch
  T X[PPT], Y[PPT], Z[PPT];
  const bool early = BUF && p == 0 && n0 > 0 && start < n0;  // (uniform)
  if (early)
    load_chunk_points<T, PPT, NT, true>(static_cast<const T *>(x0) + start, static_cast<const T *>(y0) + start,
                                        static_cast<const T *>(z0) + start, min(chunk, (int)(n0 - start)), X, Y, Z);
  EA_LM_CLOCK(t_enter_);  // (diagnostic build: kernel entered)
  const ProblemDesc pd = probs[p];
  const int active = poses[p].active;
  GroupDesc gd = {tile0_begin, tile0_end, 0, 1};
  if (p != 0) gd = groups[p];  // (uniform)
  const int evals_before = st_in[p].num_evals;
  const double state_word = lm_state_word(st_in + p, tid);
  const double cold_word = (tid & 63) < kColdWords ? reinterpret_cast<const double *>(cold_in + p)[tid & 63] : 0.0;
  double pw = 0.0;
  if constexpr (SIDE) pw = prior_word(groups, gridDim.y, p, tid);
  // ---- the step, in every workgroup: fold of the previous launch's rows + the state machine on lane 0.
  // The rows are fetched at once, beside the uniforms above and not behind them (as ea_lm_step_kernel does): a launch that
  // finds its problem finished has folded rows nobody reads and leaves below.
  reduce_tiles<NT, 8>(rows_in, gd.tile_begin, gd.tile_end, s_part, s_acc);
  asm volatile("" ::EA_DESC_UNIFORMS(T, IMG32, pd), "s"(pd.tile_begin), "s"(active), "s"(evals_before));
  if (!active) return;  // the solve of this problem ended in an earlier launch
  const bool evaluator = start < pd.n;
  if (!evaluator && !writer) return;
  const int count = evaluator ? min(chunk, (int)(pd.n - start)) : 0;
  if (evaluator && !early)  // (problems behind the first of a batch, or flat addressing: their points wait for the descriptor)
    load_chunk_points<T, PPT, NT, BUF>(static_cast<const T *>(pd.x) + start, static_cast<const T *>(pd.y) + start,
                                       static_cast<const T *>(pd.z) + start, count, X, Y, Z);
  if ((tid & 63) < kColdWords) reinterpret_cast<double *>(&s_cold[tid >> 6])[tid & 63] = cold_word;  // (own wavefront's copy)
  lm_step_park<SIDE>(state_word, pw, s_st, s_acc, tid);
  EA_LM_STAMP_PUT(0, evals_before, t_enter_);
  EA_LM_STAMP(1, evals_before);  // folded
  if (writer) {
    // ---- the writer: the full state machine on lane 0, then everything that is stored
    if (tid == 64)
      __hip_atomic_store(progress + gridDim.y + p, evals_before + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    LMPending pend;
    double acc[kAccSlots];
    if (tid == 0) {
      LMState st;
      EA_LM_STEP_LANE0(false, st, s_st, s_acc, &s_cold[0], traces + p, opt, &s_pose[0], s_trace_it, acc, pend, (void)0);
      s_store_system = pend.store_system;
    }
    __syncthreads();
    const int running = s_st.running;
    lm_step_publish(s_st, s_pose[0], st_out + p, poses + p, tid);
    // the cold system of the next launch: JtJ, Jtr of this evaluation (accepted step: lm_flush) or what this launch read
    // (rejected step); the dogleg's vectors as the state machine left them
    if (tid < kColdWords && !(s_store_system && tid < 27))
      reinterpret_cast<double *>(cold_out + p)[tid] = reinterpret_cast<const double *>(&s_cold[0])[tid];
    if (tid == 0) lm_flush(&pend, cold_out + p, traces + p, acc);
    if (!running) {
      EA_LM_STEP_DELIVER(host_states, true, s_st, s_trace_it, pend, acc, cold_out + p, traces + p, host_states + p, host_traces + p, tid);
      __syncthreads();
      if (tid == 0) __hip_atomic_store(progress + p, 0, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    // Point-sharded solve (ea_solve_sharded_comm): the rows of this launch are all-reduced over the ranks in place and the
    // next launch folds the range the widest rank needs; this rank's rows past its own stay zero -- but the all-reduce left
    // sums there two launches ago, so the writer clears them again.
    for (int r = pd.tile_end + (tid >> 5); r < gd.tile_end; r += NT / 32) rows_out[(size_t)r * kAccSlots + (tid & 31)] = 0.0;
    if (post_done && tid == 0)  // behind the flag (same lane, release order), as in ea_lm_step_kernel
      __hip_atomic_store(progress + 2 * gridDim.y + p, evals_before + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    return;
  }
  // ---- the evaluators: every WAVEFRONT takes the step itself, in the form that yields the candidate pose and nothing else
  // (lm_take_system<LITE>) -- four identical computations on four SIMDs, so the pose reaches the lanes of a wavefront without a
  // workgroup barrier: lane 0 leaves it in the wavefront's own LDS slot and its wavefront reads it back (LDS operations of one
  // wavefront execute in order).
  PoseState &s_ps = s_pose[tid >> 6];
  int running_v = 0;
  if ((tid & 63) == 0) {
    LMState st;
    LMPending pend;
    double acc[kAccSlots];
    LMCold *cold = &s_cold[tid >> 6];  // (one pointer for both arms of the macro: spelled out twice it cost the LM kernels 50 - 100 instructions)
    EA_LM_STEP_LANE0(true, st, s_st, s_acc, cold, nullptr, opt, &s_ps, s_trace_it, acc, pend,
                     EA_LM_STAMP(2, evals_before) /* state machine done */);
    running_v = st.running;
  }
  const int running = __builtin_amdgcn_readfirstlane(running_v);
  EA_LM_STAMP(3, evals_before);  // pose in LDS
  if (!running) return;  // (uniform: every workgroup of the problem arrived at the same state)
  // ---- the evaluation at the candidate pose
  if (!s_ps.unit_q) {  // (uniform, rare) the general-quaternion Jacobian reads G through the pose pointer
    if ((tid & 63) < 27) s_ps.Gf[tid & 63] = (float)s_ps.G[tid & 63];
  }
  PoseLite<T> ps;
#pragma unroll
  for (int i = 0; i < 9; ++i) ps.R[i] = uniform_scalar<T>((T)s_ps.R[i]);
#pragma unroll
  for (int i = 0; i < 3; ++i) ps.t[i] = uniform_scalar<T>((T)s_ps.t[i]);
  ps.unit_q = __builtin_amdgcn_readfirstlane(s_ps.unit_q);
  ps.full = &s_ps;
  const double sum = fused_chunk<T, PPT, 0, NT, false, BUF, IMG32, PoseLite<T>>(pd, ps, X, Y, Z, count, s_red, s_box, (T *)nullptr, 0,
                                                                            tid < kAccSlots ? tid : -1);
  EA_LM_STAMP(4, evals_before);  // evaluated
  if (tid < kAccSlots) rows_out[(size_t)(pd.tile_begin + c) * kAccSlots + tid] = sum;
#ifdef EA_STAMPS
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
  EA_LM_STAMP(5, evals_before);  // row stored
}

// q (w, x, y, z) and t of n = K x count poses, 7 doubles each -> the PoseState the evaluation kernels read, built on the
// device (ea_batch_set_poses: K different poses per problem go up as 56 bytes each instead of a 600-byte PoseState the
// host would have to compute).  Pose i belongs to problem i % count; its rotation is applied transposed for the ROS
// flavour (the problem's first term says so).
__global__ __launch_bounds__(64) void ea_make_poses_kernel(const double *__restrict__ qt, int n, int count,
                                                           const ProblemDesc *__restrict__ probs,
                                                           const GroupDesc *__restrict__ groups, PoseState *__restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  double x[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) x[k] = qt[(size_t)i * 7 + k];
  PoseState *ps = out + i;
  make_pose_state(x, probs[groups[i % count].term_begin].rot_transposed, 1, ps);
  ps->pad_[0] = 0; ps->pad_[1] = 0;
}

// pad + convert a row-major [H][W] device image into the replicated-border layout
// (dst32, inexact: fp64 problems only, nullable -- the float32 mirror of the image and a flag raised by any value the
// mirror does not hold exactly; ProblemDesc::dt32)
template <typename T>
__global__ void ea_pad_image_kernel(const T *__restrict__ src, int H, int W, T *__restrict__ dst, int pitch,
                                    float *__restrict__ dst32, int *__restrict__ inexact) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;  // padded coords
  const int v = blockIdx.y;
  if (u >= W + 2 * kImagePad) return;
  const int su = min(max(u - kImagePad, 0), W - 1);
  const int sv = min(max(v - kImagePad, 0), H - 1);
  const T val = src[(size_t)sv * W + su];
  dst[(size_t)v * pitch + u] = val;
  if (dst32) {
    const float f = (float)val;
    dst32[(size_t)v * pitch + u] = f;
    if (!((T)f == val)) atomicOr(inexact, 1);  // (also NaN)
  }
}

// The reference's Grid2D view (rows index u, columns index v: data[u * H + v], doubles; standalone_edge_align.cpp:258) ->
// the padded image in the problem's dtype: transpose, replicate the border, convert.  A 32 x 32 tile goes through LDS so
// that both the reads (v contiguous in the source) and the writes (u contiguous in the image) are coalesced.
template <typename T>
__global__ __launch_bounds__(256) void ea_grid_to_image_kernel(const double *__restrict__ grid, int W, int H, T *__restrict__ dst, int pitch,
                                                               float *__restrict__ dst32, int *__restrict__ inexact) {
  __shared__ double s_tile[32][33];
  const int PW = W + 2 * kImagePad, PH = H + 2 * kImagePad;
  const int u0 = blockIdx.x * 32, v0 = blockIdx.y * 32;   // padded coordinates of the tile
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8 threads
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    // source element (u, v): v runs with tx (contiguous in the grid), u with ty + 8 k
    const int u = u0 + ty + 8 * k, v = v0 + tx;
    const int su = min(max(u - kImagePad, 0), W - 1), sv = min(max(v - kImagePad, 0), H - 1);
    s_tile[ty + 8 * k][tx] = grid[(size_t)su * H + sv];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int v = v0 + ty + 8 * k, u = u0 + tx;
    if (v < PH && u < PW) {
      const double val = s_tile[tx][ty + 8 * k];
      dst[(size_t)v * pitch + u] = (T)val;
      if (dst32) {
        const float f = (float)val;
        dst32[(size_t)v * pitch + u] = f;
        if (!((double)f == val)) atomicOr(inexact, 1);  // (also NaN)
      }
    }
  }
}

// the reference's AoS points (columns of a_X: x y z [w] per point, doubles; utils.cpp:268-280) -> SoA in the problem's dtype
template <typename T>
__global__ __launch_bounds__(256) void ea_aos_to_soa_kernel(const double *__restrict__ src, long long n, int stride, T *__restrict__ x,
                                                            T *__restrict__ y, T *__restrict__ z) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double *s = src + i * stride;
  x[i] = (T)s[0]; y[i] = (T)s[1]; z[i] = (T)s[2];
}

// per-point weights into a problem's storage: dst[i] = (T)src[order ? order[i] : i] -- the conversion to the problem dtype
// (S = double: ea_problem_set_weights) and the tile-order permutation of the points (order[i] = caller's index of stored point i)
template <typename S, typename T>
__global__ __launch_bounds__(256) void ea_store_weights_kernel(const S *__restrict__ src, const int32_t *__restrict__ order,
                                                               long long n, T *__restrict__ dst) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  dst[i] = (T)src[order ? order[i] : i];
}

// depth weighting of a reference-frame producer (ea_problem_set_depth_weighting): w_i = min(1, (z_ref / z_i)^power) in fp64
// from the stored z: ONE division, power - 1 multiplications left to right, the min, one rounding to the problem dtype.
// The ROS scatter keeps edge pixels without a depth test, so z may be 0, negative or NaN: the clamp to [0, 1] keeps every
// stored weight a valid one (z = 0 or NaN: 1, a negative power product: 0); for z > 0 the max changes nothing.
template <typename T>
__device__ __forceinline__ void depth_weights_body(const T *__restrict__ z, long long n, double z_ref, int power, T *__restrict__ w) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double ratio = __ddiv_rn(z_ref, (double)z[i]);
  double v = ratio;
  for (int k = 1; k < power; ++k) v = __dmul_rn(v, ratio);
  w[i] = (T)fmax(0.0, fmin(1.0, v));
}
template <typename T>
__global__ __launch_bounds__(256) void ea_depth_weights_kernel(const T *__restrict__ z, long long n,
                                                               double z_ref, int power, T *__restrict__ w) {
  depth_weights_body<T>(z, n, z_ref, power, w);
}
// the same body for frame blockIdx.z of a batched producer call (ea_batch_set_frames): z, the weights behind it and the
// weighting out of the frame's slot; a frame whose problem has no depth weighting (power 0), or no point, writes nothing --
// unless its slot asks for ones (the gated multi-stream tracker: every reference carries defined weights)
template <typename T>
__global__ __launch_bounds__(256) void ea_depth_weights_frames_kernel(const FrameSlot *__restrict__ slots) {
  const FrameSlot &sl = slots[blockIdx.z];
  if (sl.power <= 0) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (sl.ones && i < (long long)sl.capacity) static_cast<T *>(sl.w)[i] = (T)1.0;
    return;
  }
  depth_weights_body<T>(static_cast<const T *>(sl.z), (long long)sl.capacity, sl.z_ref, sl.power, static_cast<T *>(sl.w));
}

// ------------------------------------------------------------------------------------------------
// Exact order statistics of |r| per residual family (ea_batch_residual_quantiles; the rules are in ea_select.h).
//
// Key pass: one lane per point of every selected family -- the projection, the four row loads and the VALUE of the bicubic
// patch (bicubic_value: the cost kernel's sample), no Jacobian row, no loss, no weight -- and |r| widened to double goes into
// the key array as its bit pattern; a failed functor leaves the all-ones key.  The plain projection serves plain and weighted
// terms (the weights do not enter, so they must not change a bit), project_point_var the distortion / second-camera functors.
// The valid blocks are not counted here: the first pass's histogram holds the count (select_valid_count) -- one integer atomic
// per wavefront on a segment's counter serialised the whole launch on one cache line (32 x 5e4 points: 224 us against 25).
template <typename T>
__global__ __launch_bounds__(kSelectThreads) void ea_select_keys_kernel(
    const ProblemDesc *__restrict__ probs, const SelectSeg *__restrict__ segs, const PoseState *__restrict__ poses,
    uint64_t *__restrict__ keys) {
  const SelectSeg sg = segs[blockIdx.y];
  const int first = blockIdx.x * kSelectThreads;
  if (first >= sg.n) return;  // (uniform)
  const ProblemDesc &pd = probs[sg.term];
  const PoseState &ps = poses[pd.group];
  const int i = first + threadIdx.x;
  if (i < sg.n) {
    bool ok;
    const T x = static_cast<const T *>(pd.x)[i], y = static_cast<const T *>(pd.y)[i], z = static_cast<const T *>(pd.z)[i];
    T fu, fv;
    int iu, iv;
    if (pd.variant & 3) {
      ProjV<T> pv;
      project_point_var<T>(pd, ps, x, y, z, pv);
      fu = pv.fu; fv = pv.fv; iu = pv.iu; iv = pv.iv; ok = pv.state == 1;
    } else {
      Proj<T> pr;
      project_point<T>(pd, ps, x, y, z, pr);
      fu = pr.fu; fv = pr.fv; iu = pr.iu; iv = pr.iv; ok = pr.state == 1;
    }
    uint64_t key = kSelectFailedKey;
    if (ok) {
      // (iu, iv are saturated to [-2, W] x [-2, H]: every tap lies inside the padded image)
      const int pitch = pd.pitch;
      const T *base = static_cast<const T *>(pd.dt) + (size_t)kImagePad * (size_t)pitch + kImagePad + (ptrdiff_t)(iv - 1) * pitch + (iu - 1);
      const T f = bicubic_value<T>(fu, fv, [&](int l) { return *reinterpret_cast<const Row4<T> *>(base + (ptrdiff_t)l * pitch); });
      key = select_key_abs((double)f);
    }
    keys[sg.begin + i] = key;
  }
}

// the key pass of ea_selftest_select: caller-supplied doubles, NaN = failed block
__global__ __launch_bounds__(kSelectThreads) void ea_select_keys_values_kernel(
    const double *__restrict__ values, const SelectSeg *__restrict__ segs, uint64_t *__restrict__ keys) {
  const SelectSeg sg = segs[blockIdx.y];
  const int first = blockIdx.x * kSelectThreads;
  if (first >= sg.n) return;  // (uniform)
  const int i = first + threadIdx.x;
  if (i < sg.n) keys[sg.begin + i] = select_key(values[sg.begin + i]);
}

// Histogram pass: a workgroup holds kSelectChunk keys of one segment in registers and, for every quantile that leads a group
// of equal prefixes, counts the keys that agree with the prefix by their digit of this pass -- integer LDS atomics -- and adds
// the bins it touched to the (segment, quantile) histogram with integer atomics: the sums do not depend on who arrives first.
__global__ __launch_bounds__(kSelectThreads) void ea_select_hist_kernel(
    const uint64_t *__restrict__ keys, const SelectSeg *__restrict__ segs, const uint64_t *__restrict__ prefix, int nq, int pass,
    unsigned *__restrict__ hist) {
  __shared__ unsigned s_hist[kSelectBins];
  static_assert(kSelectBins == kSelectChunk, "a lane owns as many bins as keys");
  const int seg = blockIdx.y, tid = threadIdx.x;
  const SelectSeg sg = segs[seg];
  const int first = blockIdx.x * kSelectChunk;
  if (first >= sg.n) return;  // (uniform)
  uint64_t k[kSelectKeysPerLane];
  unsigned have = 0;
#pragma unroll
  for (int j = 0; j < kSelectKeysPerLane; ++j) {
    const int idx = first + j * kSelectThreads + tid;
    const bool in = idx < sg.n;
    k[j] = in ? keys[sg.begin + idx] : kSelectFailedKey;
    have |= in ? 1u << j : 0u;
  }
  const uint64_t *pf = prefix + (size_t)seg * nq;
  for (int q = 0; q < nq; ++q) {
    if (select_leader(pf, q, pass) != q) continue;  // (uniform)
    const uint64_t want = pf[q];
#pragma unroll
    for (int j = 0; j < kSelectKeysPerLane; ++j) s_hist[j * kSelectThreads + tid] = 0;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kSelectKeysPerLane; ++j)
      if (((have >> j) & 1u) && select_matches(k[j], want, pass)) atomicAdd(&s_hist[select_digit(k[j], pass)], 1u);
    __syncthreads();
    unsigned *h = hist + ((size_t)seg * nq + q) * kSelectBins;
#pragma unroll
    for (int j = 0; j < kSelectKeysPerLane; ++j) {
      const unsigned c = s_hist[j * kSelectThreads + tid];
      if (c) atomicAdd(&h[j * kSelectThreads + tid], c);
    }
    __syncthreads();
  }
}

// Scan: one workgroup per segment.  Per quantile the 2048 bins of its leader's histogram are summed 8 to a lane and 16 lanes
// to a group, and lane 0 walks 16 groups, 16 lanes, 8 bins (select_scan) to the bin that holds the rank; the prefix takes the
// digit, the rank becomes the rank inside the bin.  Pass 0 reads the number of valid blocks off its histogram (every quantile
// shares it then: the keys with the top bit clear), keeps it in n_valid and turns the probabilities into ranks; the last pass
// writes the values.  The histograms are left zeroed for the next pass.
__global__ __launch_bounds__(kSelectThreads) void ea_select_scan_kernel(
    const double *__restrict__ probs, int nq, int pass, unsigned *__restrict__ n_valid, uint64_t *prefix, int64_t *rank,
    unsigned *hist, double *__restrict__ out_values, int64_t *__restrict__ out_n_valid) {
  __shared__ unsigned s1[kSelectThreads];
  __shared__ unsigned s2[16];
  __shared__ int s_leader[kSelectMaxQ];
  __shared__ uint64_t s_old[kSelectMaxQ];
  static_assert(kSelectBins == 8 * kSelectThreads && kSelectThreads == 16 * 16, "8 bins a lane, 16 lanes a group, 16 groups");
  const int seg = blockIdx.x, tid = threadIdx.x;
  uint64_t *pf = prefix + (size_t)seg * nq;
  int64_t *rk = rank + (size_t)seg * nq;
  int64_t m = pass == 0 ? 0 : (int64_t)n_valid[seg];  // (lane 0's alone from here on)
  if (tid < nq) {
    s_leader[tid] = select_leader(pf, tid, pass);
    s_old[tid] = pass == 0 ? 0 : pf[tid];
  }
  __syncthreads();
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  for (int q = 0; q < nq; ++q) {
    const unsigned *h = hist + ((size_t)seg * nq + s_leader[q]) * kSelectBins;
    const u32x4 a = reinterpret_cast<const u32x4 *>(h)[2 * tid], b = reinterpret_cast<const u32x4 *>(h)[2 * tid + 1];
    s1[tid] = a.x + a.y + a.z + a.w + b.x + b.y + b.z + b.w;
    __syncthreads();
    if (tid < 16) {
      unsigned s = 0;
#pragma unroll
      for (int j = 0; j < 16; ++j) s += s1[16 * tid + j];
      s2[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
      if (pass == 0) {
        m = select_valid_count(s2);
        if (q == 0) n_valid[seg] = (unsigned)m;
      }
      int64_t r = pass == 0 ? select_rank(probs[q], m) : rk[q];
      const int i2 = select_scan(s2, 16, r, &r);
      const int i1 = select_scan(s1 + 16 * i2, 16, r, &r);
      const int lane = 16 * i2 + i1;
      const int bin = 8 * lane + select_scan(h + 8 * lane, 8, r, &r);
      const uint64_t key = select_extend(s_old[q], pass, (unsigned)bin);
      pf[q] = key;
      rk[q] = r;
      if (pass == kSelectPasses - 1) {
        out_values[(size_t)seg * nq + q] = m > 0 ? select_value(key) : __builtin_nan("");
        if (q == 0) out_n_valid[seg] = m;
      }
    }
    __syncthreads();
  }
  for (int q = 0; q < nq; ++q) {
    if (s_leader[q] != q) continue;
    u32x4 *h = reinterpret_cast<u32x4 *>(hist + ((size_t)seg * nq + q) * kSelectBins);
    const u32x4 zero = {0u, 0u, 0u, 0u};
    h[2 * tid] = zero;
    h[2 * tid + 1] = zero;
  }
}

// ------------------------------------------------------------------------------------------------
// How much of a reference is seen at a pose (ea_batch_pose_stats; the definitions are in ea_hip.h).
//
// Shaped like the key pass above: one lane per point, blockIdx.y the problem's segment (sg.begin: its first partial row).
// Per lane the projection at the pose, the visibility test on the saturated floor -- -2 and W / H, where the saturation
// sets in, lie outside every accepted range, so the test is the unsaturated one's -- and for a visible point the four row
// loads, the bicubic value and the projection at the identity (R = I, t = 0 in the kernel's type: what the pose kernel makes
// of q = (1, 0, 0, 0), so the flow at the identity is exactly 0).  The divisor's sign is read off its reciprocal: 0 < iz <
// Inf.  Counts: a ballot and a popcount per wavefront.  The flow: the fixed xor butterfly of the wavefront, then the four
// wavefronts in order.  ONE partial row per workgroup, no atomics: a segment's partials depend on its own points alone.
template <typename T>
__device__ __forceinline__ bool pose_stats_project(const ProblemDesc &pd, const PoseLite<T> &ps, T x, T y, T z, T &u, T &v, T &fu,
                                                   T &fv, int &iu, int &iv, bool &front) {
  T iz;
  bool ok;
  if (pd.variant & 3) {
    ProjV<T> pv;
    project_point_var<T>(pd, ps, x, y, z, pv);
    u = pv.u; v = pv.v; fu = pv.fu; fv = pv.fv; iu = pv.iu; iv = pv.iv; iz = pv.iz; ok = pv.state == 1;
  } else {
    Proj<T> pr;
    project_point<T>(pd, ps, x, y, z, pr);
    u = pr.u; v = pr.v; fu = pr.fu; fv = pr.fv; iu = pr.iu; iv = pr.iv; iz = pr.iz; ok = pr.state == 1;
  }
  front = iz > T(0) && iz < (T)__builtin_inf();
  return ok;
}

template <typename T>
__global__ __launch_bounds__(kPoseStatsThreads) void ea_pose_stats_kernel(
    const ProblemDesc *__restrict__ probs, const SelectSeg *__restrict__ segs, const PoseState *__restrict__ poses, int margin,
    double inlier_residual, PoseStatsPartial *__restrict__ partials) {
  __shared__ int s_cnt[kPoseStatsThreads / 64][4];
  __shared__ double s_sum[kPoseStatsThreads / 64];
  const SelectSeg sg = segs[blockIdx.y];
  const int first = blockIdx.x * kPoseStatsThreads;
  if (first >= sg.n) return;  // (uniform)
  const ProblemDesc &pd = probs[sg.term];
  const PoseState &full = poses[pd.group];
  const int tid = threadIdx.x, i = first + tid;
  bool invalid = false, visible = false, inlier = false, flow = false;
  double dist = 0.0;
  if (i < sg.n) {
    PoseLite<T> at, id;
#pragma unroll
    for (int k = 0; k < 9; ++k) { at.R[k] = Uni<T>::R(full)[k]; id.R[k] = (k % 4 == 0) ? T(1) : T(0); }
#pragma unroll
    for (int k = 0; k < 3; ++k) { at.t[k] = Uni<T>::t(full)[k]; id.t[k] = T(0); }
    at.unit_q = id.unit_q = 1;  // (no Jacobian here)
    at.full = id.full = &full;
    const T x = static_cast<const T *>(pd.x)[i], y = static_cast<const T *>(pd.y)[i], z = static_cast<const T *>(pd.z)[i];
    T u, v, fu, fv;
    int iu, iv;
    bool front;
    const bool ok = pose_stats_project<T>(pd, at, x, y, z, u, v, fu, fv, iu, iv, front);
    invalid = !ok;
    visible = ok && front && iu >= margin && iu <= pd.W - 2 - margin && iv >= margin && iv <= pd.H - 2 - margin;
    if (visible) {
      const int pitch = pd.pitch;
      const T *base = static_cast<const T *>(pd.dt) + (size_t)kImagePad * (size_t)pitch + kImagePad + (ptrdiff_t)(iv - 1) * pitch + (iu - 1);
      const T f = bicubic_value<T>(fu, fv, [&](int l) { return *reinterpret_cast<const Row4<T> *>(base + (ptrdiff_t)l * pitch); });
      inlier = fabs((double)f) <= inlier_residual;
      T u0, v0, fu0, fv0;
      int iu0, iv0;
      bool front0;
      const bool ok0 = pose_stats_project<T>(pd, id, x, y, z, u0, v0, fu0, fv0, iu0, iv0, front0);
      flow = ok0 && front0;
      if (flow) {
        const double du = (double)u - (double)u0, dv = (double)v - (double)v0;
        dist = sqrt(fma(du, du, dv * dv));
      }
    }
  }
  const int lane = tid & 63, wave = tid >> 6;
  const int c0 = __popcll(__builtin_amdgcn_ballot_w64(invalid)), c1 = __popcll(__builtin_amdgcn_ballot_w64(visible));
  const int c2 = __popcll(__builtin_amdgcn_ballot_w64(inlier)), c3 = __popcll(__builtin_amdgcn_ballot_w64(flow));
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) dist += __shfl_xor(dist, m, 64);
  if (lane == 0) {
    s_cnt[wave][0] = c0; s_cnt[wave][1] = c1; s_cnt[wave][2] = c2; s_cnt[wave][3] = c3;
    s_sum[wave] = dist;
  }
  __syncthreads();
  if (tid == 0) {
    PoseStatsPartial o = {0, 0, 0, 0, 0.0, 0.0};
#pragma unroll
    for (int w = 0; w < kPoseStatsThreads / 64; ++w) {
      o.n_invalid += s_cnt[w][0]; o.n_visible += s_cnt[w][1]; o.n_inlier += s_cnt[w][2]; o.n_flow += s_cnt[w][3];
      o.sum_flow += s_sum[w];
    }
    partials[sg.begin + blockIdx.x] = o;
  }
}

// the fold: one wavefront per segment; lane L takes the partials L, L + 64, ... in that order, then the same butterfly.  The
// order is a function of the segment's point count alone.
__global__ __launch_bounds__(64) void ea_pose_stats_fold_kernel(const SelectSeg *__restrict__ segs,
                                                                  const PoseStatsPartial *__restrict__ partials,
                                                                  PoseStatsRow *__restrict__ out) {
  const SelectSeg sg = segs[blockIdx.x];
  const int rows = (sg.n + kPoseStatsThreads - 1) / kPoseStatsThreads, lane = threadIdx.x;
  long long c0 = 0, c1 = 0, c2 = 0, c3 = 0;
  double sum = 0.0;
  for (int k = lane; k < rows; k += 64) {
    const PoseStatsPartial p = partials[sg.begin + k];
    c0 += p.n_invalid; c1 += p.n_visible; c2 += p.n_inlier; c3 += p.n_flow;
    sum += p.sum_flow;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    c0 += __shfl_xor(c0, m, 64); c1 += __shfl_xor(c1, m, 64); c2 += __shfl_xor(c2, m, 64); c3 += __shfl_xor(c3, m, 64);
    sum += __shfl_xor(sum, m, 64);
  }
  if (lane == 0) out[blockIdx.x] = PoseStatsRow{(int64_t)sg.n, (int64_t)c0, (int64_t)c1, (int64_t)c2, (int64_t)c3, sum};
}

// ------------------------------------------------------------------------------------------------
// The reference's qualitative self-check: reproject (standalone/utils.cpp:497-592, all four overloads) and s_overlay
// (:594-608).  ea_hip.h states the arithmetic; like ea_pixel_cost_kernel it is fp64 from the stored points widened to double,
// in the stated operation order, IEEE divisions, nothing contracted.
//
// Shaped like ea_pose_stats_kernel: one lane per point, blockIdx.y the segment (one per problem of the call), the segment's
// 3x4 matrix -- built on the host, the rig product included -- and the descriptor uniform per workgroup.  No validity test:
// bz == 0 and points behind the camera give what IEEE gives.
//   PAINT = false: (u, v) leaves as one 16-byte store per lane at row sg.row + i, the storage order of the rows layout.
//   PAINT = true:  pixel ((int)v, (int)u) of the segment's image takes the colour when the point is inside by
//     ea_pixel_cost_kernel's rule, else it is counted outside.  Points that share a pixel store the same three bytes.  Counts:
//     a ballot and a popcount per wavefront, the four wavefronts summed, ONE integer atomic pair per workgroup on the
//     segment's two counters {inside, outside} (exact whatever the order of arrival).
template <typename T, bool PAINT>
__global__ __launch_bounds__(kReprojectThreads) void ea_reproject_kernel(const ProblemDesc *__restrict__ probs,
                                                                         const ReprojectSeg *__restrict__ segs,
                                                                         double *__restrict__ uv, unsigned int color,
                                                                         unsigned long long *__restrict__ counts) {
  __shared__ int s_cnt[kReprojectThreads / 64][2];
  const ReprojectSeg &sg = segs[blockIdx.y];
  const int n = sg.n;
  const int first = blockIdx.x * kReprojectThreads;
  if (first >= n) return;  // (uniform)
  const ProblemDesc &pd = probs[sg.term];
  const int tid = threadIdx.x, i = first + tid;
  bool inside = false, outside = false;
  if (i < n) {
    const double x = (double)static_cast<const T *>(pd.x)[i], y = (double)static_cast<const T *>(pd.y)[i],
                 z = (double)static_cast<const T *>(pd.z)[i];
    const double *M = sg.M;
    double u, v;
    {
#pragma clang fp contract(off)
      const double bx = ((M[0] * x + M[1] * y) + M[2] * z) + M[3];
      const double by = ((M[4] * x + M[5] * y) + M[6] * z) + M[7];
      const double bz = ((M[8] * x + M[9] * y) + M[10] * z) + M[11];
      double xd = bx / bz, yd = by / bz;
      if (pd.variant & 1) {  // coefficients by name: k1, k2, p1, p2, k3 (ea_problem_set_distortion)
        const double k1 = pd.dist[0], k2 = pd.dist[1], p1 = pd.dist[2], p2 = pd.dist[3], k3 = pd.dist[4];
        const double xn = xd, yn = yd;
        const double r2 = xn * xn + yn * yn, r4 = r2 * r2, r6 = r4 * r2;
        const double rad = ((1.0 + k1 * r2) + k2 * r4) + k3 * r6;
        xd = (xn * rad + ((2.0 * p1) * xn) * yn) + p2 * (r2 + (2.0 * xn) * xn);
        yd = (yn * rad + ((2.0 * p2) * xn) * yn) + p1 * (r2 + (2.0 * yn) * yn);
      }
      u = pd.fx * xd + pd.cx;
      v = pd.fy * yd + pd.cy;
    }
    if (!PAINT) {
      typedef double D2 __attribute__((ext_vector_type(2)));
      reinterpret_cast<D2 *>(uv)[sg.row + i] = D2{u, v};
    } else {
      const bool finite = (u == u) && (v == v) && fabs(u) < 1e9 && fabs(v) < 1e9;
      const int iu = finite ? (int)u : -1, iv = finite ? (int)v : -1;  // `(int)`: truncation toward zero
      inside = finite && iu >= 0 && iu < pd.W && iv >= 0 && iv < pd.H && !(u <= -1.0) && !(v <= -1.0);
      outside = !inside;
      unsigned char *img = sg.image;
      if (inside && img) {
        unsigned char *px = img + ((size_t)iv * (size_t)pd.W + (size_t)iu) * 3;
        px[0] = (unsigned char)(color & 0xffu);
        px[1] = (unsigned char)((color >> 8) & 0xffu);
        px[2] = (unsigned char)((color >> 16) & 0xffu);
      }
    }
  }
  if (PAINT) {
    const int lane = tid & 63, wave = tid >> 6;
    const int c0 = __popcll(__builtin_amdgcn_ballot_w64(inside)), c1 = __popcll(__builtin_amdgcn_ballot_w64(outside));
    if (lane == 0) { s_cnt[wave][0] = c0; s_cnt[wave][1] = c1; }
    __syncthreads();
    if (tid == 0) {
      int nin = 0, nout = 0;
#pragma unroll
      for (int w = 0; w < kReprojectThreads / 64; ++w) { nin += s_cnt[w][0]; nout += s_cnt[w][1]; }
      if (nin) atomicAdd(&counts[2 * blockIdx.y], (unsigned long long)nin);
      if (nout) atomicAdd(&counts[2 * blockIdx.y + 1], (unsigned long long)nout);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// The depth-consistency gate (ea_*_depth_gate): every warped point's depth against the depth measured where it lands in the
// current frame.  ea_hip.h states the arithmetic and ea_depth_gate.h holds it (gate_point: the projection of step B, the
// inside rule, the window scan, the classification; fp64, nothing contracted), shared with the host shim.
//
// Shaped like ea_reproject_kernel: one lane per stored point, blockIdx.y the segment (one per problem of the call), the
// segment -- its 3x4 matrix, depth image, weights and class pointers -- the descriptor and the rule uniform per workgroup.
// RAW is the depth kind (uint16_t / float), R the window radius: the (2 R + 1)^2 window is that many independent 2- or 4-byte
// gather loads per lane (a pixel outside the image reads pixel 0 and counts as "no measurement"), all issued before the
// compare chain; a VGA depth image is 0.6-1.2 MB and stays in L2.  The depth image may be 2^shift times the DT extent (step
// 3b; the shift a run-time value of the segment, uniform per workgroup: two scalar shifts, and per lane and axis one multiplication and one addition).  Per lane one coalesced weight store (apply) and one byte
// store (classes asked for).  Counts: six ballots and popcounts per wavefront, the four wavefronts summed through LDS, at most
// six integer atomics per workgroup on the segment's counters (exact whatever the order of arrival).
template <typename T, typename RAW, int R>
__global__ __launch_bounds__(kDepthGateThreads) void ea_depth_gate_kernel(const ProblemDesc *__restrict__ probs,
                                                                          const DepthGateSeg *__restrict__ segs, DepthGateRule rule,
                                                                          unsigned long long *__restrict__ counts) {
  __shared__ int s_cnt[kDepthGateThreads / 64][kDepthGateClasses];
  const DepthGateSeg &sg = segs[blockIdx.y];
  const int n = sg.n;
  const int first = blockIdx.x * kDepthGateThreads;
  if (first >= n) return;  // (uniform)
  const ProblemDesc &pd = probs[sg.term];
  const int tid = threadIdx.x, i = first + tid;
  int cls = -1;
  if (i < n) {
    typedef T __attribute__((address_space(1))) *GOutT;
    typedef unsigned char __attribute__((address_space(1))) *GOutB;
    const double x = (double)((GPtr<T>)static_cast<const T *>(pd.x))[i], y = (double)((GPtr<T>)static_cast<const T *>(pd.y))[i],
                 z = (double)((GPtr<T>)static_cast<const T *>(pd.z))[i];
    cls = gate_point<RAW, R, GPtr<RAW>>(sg.M, x, y, z, pd.fx, pd.fy, pd.cx, pd.cy, (pd.variant & 1) ? pd.dist : nullptr,
                                        (GPtr<RAW>)static_cast<const RAW *>(sg.depth), pd.H, pd.W, sg.z_scaling, rule.abs_tol,
                                        rule.rel_tol, sg.shift);
    if (sg.cls) ((GOutB)sg.cls)[i] = (unsigned char)cls;
    if (sg.weights)
      ((GOutT) static_cast<T *>(sg.weights))[i] = (T)gate_weight(gate_factor(rule, cls), gate_depth_factor(z, sg.dw_z_ref, sg.dw_power));
  }
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int c = 0; c < kDepthGateClasses; ++c) {
    const int cnt = __popcll(__builtin_amdgcn_ballot_w64(cls == c));
    if (lane == 0) s_cnt[wave][c] = cnt;
  }
  __syncthreads();
  if (tid < kDepthGateClasses) {
    int sum = 0;
#pragma unroll
    for (int w = 0; w < kDepthGateThreads / 64; ++w) sum += s_cnt[w][tid];
    if (sum) atomicAdd(&counts[(size_t)kDepthGateClasses * blockIdx.y + tid], (unsigned long long)sum);
  }
}

// ------------------------------------------------------------------------------------------------
// Point selection (ea_*_select_points): the reference's stride and one point per cell, on the points a problem holds.
// ea_hip.h states the rule and ea_point_select.h holds it (select_pixel, select_cell; fp64, nothing contracted), shared with
// the host shim.
//
// Shaped like ea_depth_gate_kernel: one lane per stored point, blockIdx.y the segment (one per problem of the call), the
// segment uniform per workgroup.  The passes of a call, in stream order:
//   keys (cell_px > 0)  NEAREST first: atomicMin of the bits of z into the segment's 64-bit cell table (positive doubles order
//                       like their bit patterns).  Then every rule: atomicMin of the point index into the 32-bit cell table,
//                       from all points of the cell, or for NEAREST from those whose z bits are the cell's minimum.  Minima of
//                       integers: the same tables whatever the order of arrival.  The tables are all ones before the pass.
//   count               a point is flagged when it won its cell, or has no pixel and `outside` keeps those (cell_px == 0: every
//                       point).  A ballot and a popcount per wavefront, the four wavefronts summed through LDS: one count per
//                       workgroup, and ONE integer atomic per workgroup on the segment's no_pixel counter.
//   scan                one workgroup per segment turns its counts into offsets, 1024 at a time with a carry between the
//                       chunks (ea_edge_scan_kernel's pattern), and leaves the total: the survivors of the cell step.
//   compact             the flags again (the tables are unchanged), ordinal = block offset + wave prefix + lane rank; the point
//                       is kept iff ordinal % stride_used == 0 and goes to slot ordinal / stride_used of the segment's new
//                       arrays: x, y, z and the weight, as stored, by plain vector stores.
// Ordinals and strides fit 32 bits: a problem holds fewer than 2^31 points, and the host clamps stride and target to 2^31 - 1,
// which no ordinal reaches.
template <typename T>
__device__ __forceinline__ bool point_select_pixel(const PointSelectSeg &sg, int i, int cell_px, int *cell, unsigned long long *zbits) {
  const double x = (double)((GPtr<T>)static_cast<const T *>(sg.x))[i], y = (double)((GPtr<T>)static_cast<const T *>(sg.y))[i],
               z = (double)((GPtr<T>)static_cast<const T *>(sg.z))[i];
  int pu, pv;
  const bool has = select_pixel(x, y, z, sg.fx, sg.fy, sg.cx, sg.cy, sg.height, sg.width, &pu, &pv);
  *cell = has ? select_cell(pu, pv, cell_px, sg.cells_x) : 0;
  *zbits = (unsigned long long)__double_as_longlong(z);
  return has;
}

// PASS 0: the cells' smallest z bits (NEAREST only).  PASS 1: the cells' winning index
template <typename T, int PASS>
__global__ __launch_bounds__(kPointSelectThreads) void ea_point_select_keys_kernel(const PointSelectSeg *__restrict__ segs, int cell_px,
                                                                                   int nearest) {
  const PointSelectSeg &sg = segs[blockIdx.y];
  const int i = blockIdx.x * kPointSelectThreads + threadIdx.x;
  if (i >= sg.n) return;
  int cell;
  unsigned long long zbits;
  if (!point_select_pixel<T>(sg, i, cell_px, &cell, &zbits)) return;
  if (PASS == 0) atomicMin(&sg.zmin[cell], zbits);
  else if (!nearest || sg.zmin[cell] == zbits) atomicMin(&sg.imin[cell], (unsigned int)i);
}

template <typename T>
__device__ __forceinline__ bool point_select_flag(const PointSelectSeg &sg, int i, int cell_px, int outside, bool *no_pixel) {
  *no_pixel = false;
  if (cell_px == 0) return true;  // (uniform)
  int cell;
  unsigned long long zbits;
  if (!point_select_pixel<T>(sg, i, cell_px, &cell, &zbits)) { *no_pixel = true; return outside != 0; }
  return sg.imin[cell] == (unsigned int)i;
}

template <typename T>
__global__ __launch_bounds__(kPointSelectThreads) void ea_point_select_count_kernel(const PointSelectSeg *__restrict__ segs, int cell_px,
                                                                                    int outside, PointSelectOut *__restrict__ out) {
  __shared__ int s_cnt[kPointSelectThreads / 64][2];
  const PointSelectSeg &sg = segs[blockIdx.y];
  const int n = sg.n;
  const int first = blockIdx.x * kPointSelectThreads;
  if (first >= n) return;  // (uniform)
  const int tid = threadIdx.x, i = first + tid;
  bool flag = false, none = false;
  if (i < n) flag = point_select_flag<T>(sg, i, cell_px, outside, &none);
  const int lane = tid & 63, wave = tid >> 6;
  const int c0 = __popcll(__builtin_amdgcn_ballot_w64(flag)), c1 = __popcll(__builtin_amdgcn_ballot_w64(none));
  if (lane == 0) { s_cnt[wave][0] = c0; s_cnt[wave][1] = c1; }
  __syncthreads();
  if (tid == 0) {
    int kept = 0, nopix = 0;
#pragma unroll
    for (int w = 0; w < kPointSelectThreads / 64; ++w) { kept += s_cnt[w][0]; nopix += s_cnt[w][1]; }
    sg.block_counts[blockIdx.x] = kept;
    if (nopix) atomicAdd(&out[blockIdx.y].no_pixel, (unsigned long long)nopix);
  }
}

// exclusive scan of a segment's block counts by one workgroup, sequential over chunks of 1024 with a carry
__global__ __launch_bounds__(kPointSelectScan) void ea_point_select_scan_kernel(const PointSelectSeg *__restrict__ segs,
                                                                                PointSelectOut *__restrict__ out) {
  __shared__ int s_buf[kPointSelectScan];
  __shared__ int s_carry;
  const PointSelectSeg &sg = segs[blockIdx.x];
  const int nblocks = (sg.n + kPointSelectThreads - 1) / kPointSelectThreads;
  int *counts = sg.block_counts;
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  for (int base = 0; base < nblocks; base += kPointSelectScan) {
    const int i = base + threadIdx.x;
    const int v = i < nblocks ? counts[i] : 0;
    s_buf[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < kPointSelectScan; off <<= 1) {  // Hillis-Steele inclusive scan
      const int t = threadIdx.x >= off ? s_buf[threadIdx.x - off] : 0;
      __syncthreads();
      s_buf[threadIdx.x] += t;
      __syncthreads();
    }
    const int incl = s_buf[threadIdx.x], carry = s_carry;
    if (i < nblocks) counts[i] = carry + incl - v;
    __syncthreads();
    if (threadIdx.x == kPointSelectScan - 1) s_carry = carry + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x].after_cells = s_carry;
}

template <typename T>
__global__ __launch_bounds__(kPointSelectThreads) void ea_point_select_compact_kernel(const PointSelectSeg *__restrict__ segs, int cell_px,
                                                                                      int outside, unsigned int stride, unsigned int target,
                                                                                      const PointSelectOut *__restrict__ out) {
  __shared__ int s_cnt[kPointSelectThreads / 64];
  const PointSelectSeg &sg = segs[blockIdx.y];
  const int n = sg.n;
  const int first = blockIdx.x * kPointSelectThreads;
  if (first >= n) return;  // (uniform)
  const int tid = threadIdx.x, i = first + tid;
  bool flag = false, none;
  if (i < n) flag = point_select_flag<T>(sg, i, cell_px, outside, &none);
  const int lane = tid & 63, wave = tid >> 6;
  const unsigned long long m = __builtin_amdgcn_ballot_w64(flag);
  if (lane == 0) s_cnt[wave] = __popcll(m);
  __syncthreads();
  if (!flag) return;
  unsigned int ordinal = (unsigned int)sg.block_counts[blockIdx.x];
  for (int w = 0; w < wave; ++w) ordinal += (unsigned int)s_cnt[w];
  ordinal += (unsigned int)__popcll(m & ((1ull << lane) - 1ull));
  const unsigned int survivors = (unsigned int)out[blockIdx.y].after_cells;
  const unsigned int s = (unsigned int)select_stride_used((int64_t)survivors, (int64_t)stride, (int64_t)target);
  const unsigned int slot = ordinal / s;
  if (slot * s != ordinal) return;
  typedef T __attribute__((address_space(1))) *GOutT;
  const GPtr<T> gz = (GPtr<T>)static_cast<const T *>(sg.z);
  const GOutT goz = (GOutT) static_cast<T *>(sg.oz);
  ((GOutT) static_cast<T *>(sg.ox))[slot] = ((GPtr<T>)static_cast<const T *>(sg.x))[i];
  ((GOutT) static_cast<T *>(sg.oy))[slot] = ((GPtr<T>)static_cast<const T *>(sg.y))[i];
  goz[slot] = gz[i];
  if (sg.weighted) goz[sg.w_out + slot] = gz[sg.w_in + i];
}
// ------------------------------------------------------------------------------------------------
// Carrying reference points between frames (ea_*_transform_points, ea_*_merge_points).  ea_hip.h states the rule and
// ea_point_merge.h holds it (merge_transform, merge_pixel, merge_weight on top of ea_point_select.h's select_pixel and
// select_cell; fp64, nothing contracted), shared with the host shim.
//
// Shaped like the point selection passes: one lane per stored point, blockIdx.y the segment (one per problem of the call), the
// segment uniform per workgroup.  ea_point_transform_kernel rewrites a problem's points in place: a lane reads its own point,
// then writes it.  The passes of a merge, in stream order:
//   occupancy (cell_px > 0)  every dst point that has a pixel clears its cell's byte (all ones before the pass): plain stores
//                            of one value, the same table whatever the order of arrival.
//   keys (cell_px > 0)       over the src points that pass steps 1-3 and whose cell is free: NEAREST first the atomicMin of the
//                            bits of z' (positive doubles order like their bit patterns), then every rule the atomicMin of the
//                            src index.  Minima of integers.
//   count                    steps 1-4 again; a ballot and a popcount per wavefront, summed through LDS: one count of survivors
//                            per workgroup, and at most one integer atomic per workgroup and counter of the segment.
//   scan                     ea_point_select_scan_kernel on the block counts: offsets, and the survivors of the segment.
//   copy                     workgroups [0, dst_blocks): dst's points as stored to the front of the new arrays, its weights or
//                            exactly 1.  Workgroups behind them: a surviving src point whose ordinal is below the cap goes to
//                            slot n_dst + ordinal -- the rounded x', y', z' and w_src * weight_scale.  Plain vector stores.
template <typename T>
__global__ __launch_bounds__(kPointMergeThreads) void ea_point_transform_kernel(const PointTransformSeg *__restrict__ segs) {
  const PointTransformSeg &sg = segs[blockIdx.y];
  const int i = blockIdx.x * kPointMergeThreads + threadIdx.x;
  if (i >= sg.n) return;
  typedef T __attribute__((address_space(1))) *GOutT;
  const GOutT gx = (GOutT) static_cast<T *>(sg.x), gy = (GOutT) static_cast<T *>(sg.y), gz = (GOutT) static_cast<T *>(sg.z);
  double ox, oy, oz;
  merge_transform(sg.M, (double)gx[i], (double)gy[i], (double)gz[i], &ox, &oy, &oz);
  gx[i] = (T)ox; gy[i] = (T)oy; gz[i] = (T)oz;
}

// what steps 1-3 make of src point i: 0 a candidate (pu, pv, cell and the bits of z' set where a pixel was asked for),
// 1 no pixel, 2 off the edges.  The rounded point comes back in r[3]
template <typename T>
__device__ __forceinline__ int point_merge_candidate(const PointMergeSeg &sg, int i, int need_pixel, int margin, double max_dt, int cell_px,
                                                     T r[3], int *cell, unsigned long long *zbits) {
  double ox, oy, oz;
  merge_transform(sg.M, (double)((GPtr<T>)static_cast<const T *>(sg.sx))[i], (double)((GPtr<T>)static_cast<const T *>(sg.sy))[i],
                  (double)((GPtr<T>)static_cast<const T *>(sg.sz))[i], &ox, &oy, &oz);
  r[0] = (T)ox; r[1] = (T)oy; r[2] = (T)oz;
  *cell = 0;
  *zbits = (unsigned long long)__double_as_longlong((double)r[2]);
  if (!need_pixel) return 0;  // (uniform)
  int pu, pv;
  if (!merge_pixel((double)r[0], (double)r[1], (double)r[2], sg.fx, sg.fy, sg.cx, sg.cy, sg.height, sg.width, margin, &pu, &pv)) return 1;
  if (max_dt >= 0.0) {
    const double d = (double)((GPtr<T>)static_cast<const T *>(sg.dt))[(size_t)(pv + kImagePad) * (size_t)sg.pitch + (size_t)(pu + kImagePad)];
    if (!(d <= max_dt)) return 2;  // (NaN fails)
  }
  if (cell_px > 0) *cell = select_cell(pu, pv, cell_px, sg.cells_x);
  return 0;
}

template <typename T>
__global__ __launch_bounds__(kPointMergeThreads) void ea_point_merge_occupancy_kernel(const PointMergeSeg *__restrict__ segs, int cell_px) {
  const PointMergeSeg &sg = segs[blockIdx.y];
  const int i = blockIdx.x * kPointMergeThreads + threadIdx.x;
  if (i >= sg.n_dst) return;
  int pu, pv;
  if (!select_pixel((double)((GPtr<T>)static_cast<const T *>(sg.x))[i], (double)((GPtr<T>)static_cast<const T *>(sg.y))[i],
                    (double)((GPtr<T>)static_cast<const T *>(sg.z))[i], sg.fx, sg.fy, sg.cx, sg.cy, sg.height, sg.width, &pu, &pv))
    return;
  sg.occ[select_cell(pu, pv, cell_px, sg.cells_x)] = 0;
}

// PASS 0: the free cells' smallest z' bits (NEAREST only).  PASS 1: the free cells' winning src index
template <typename T, int PASS>
__global__ __launch_bounds__(kPointMergeThreads) void ea_point_merge_keys_kernel(const PointMergeSeg *__restrict__ segs, int margin,
                                                                                 double max_dt, int cell_px, int nearest) {
  const PointMergeSeg &sg = segs[blockIdx.y];
  const int i = blockIdx.x * kPointMergeThreads + threadIdx.x;
  if (i >= sg.n_src) return;
  T r[3];
  int cell;
  unsigned long long zbits;
  if (point_merge_candidate<T>(sg, i, 1, margin, max_dt, cell_px, r, &cell, &zbits) != 0) return;
  if (sg.occ[cell] == 0) return;
  if (PASS == 0) atomicMin(&sg.zmin[cell], zbits);
  else if (!nearest || sg.zmin[cell] == zbits) atomicMin(&sg.imin[cell], (unsigned int)i);
}

// steps 1-4 of src point i: 0 survives, 1 no pixel, 2 off the edges, 3 its cell is occupied, 4 it lost its cell
template <typename T>
__device__ __forceinline__ int point_merge_fate(const PointMergeSeg &sg, int i, int need_pixel, int margin, double max_dt, int cell_px, T r[3]) {
  int cell;
  unsigned long long zbits;
  const int c = point_merge_candidate<T>(sg, i, need_pixel, margin, max_dt, cell_px, r, &cell, &zbits);
  if (c != 0 || cell_px == 0) return c;
  if (sg.occ[cell] == 0) return 3;
  return sg.imin[cell] == (unsigned int)i ? 0 : 4;
}

template <typename T>
__global__ __launch_bounds__(kPointMergeThreads) void ea_point_merge_count_kernel(const PointMergeSeg *__restrict__ segs, int need_pixel,
                                                                                  int margin, double max_dt, int cell_px,
                                                                                  PointMergeOut *__restrict__ out) {
  __shared__ int s_cnt[kPointMergeThreads / 64][5];
  const PointMergeSeg &sg = segs[blockIdx.y];
  const int n = sg.n_src;
  const int first = blockIdx.x * kPointMergeThreads;
  if (first >= n) return;  // (uniform)
  const int tid = threadIdx.x, i = first + tid;
  int fate = -1;
  T r[3];
  if (i < n) fate = point_merge_fate<T>(sg, i, need_pixel, margin, max_dt, cell_px, r);
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const int c = __popcll(__builtin_amdgcn_ballot_w64(fate == k));
    if (lane == 0) s_cnt[wave][k] = c;
  }
  __syncthreads();
  if (tid < 5) {
    int sum = 0;
#pragma unroll
    for (int w = 0; w < kPointMergeThreads / 64; ++w) sum += s_cnt[w][tid];
    if (tid == 0) sg.block_counts[blockIdx.x] = sum;
    else if (sum) {
      PointMergeOut &o = out[blockIdx.y];
      unsigned long long *slot = tid == 1 ? &o.no_pixel : tid == 2 ? &o.off_edge : tid == 3 ? &o.occupied : &o.lost_cell;
      atomicAdd(slot, (unsigned long long)sum);
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kPointMergeThreads) void ea_point_merge_copy_kernel(const PointMergeSeg *__restrict__ segs, int dst_blocks,
                                                                                 int need_pixel, int margin, double max_dt, int cell_px,
                                                                                 unsigned int cap, double weight_scale) {
  __shared__ int s_cnt[kPointMergeThreads / 64];
  typedef T __attribute__((address_space(1))) *GOutT;
  const PointMergeSeg &sg = segs[blockIdx.y];
  const int tid = threadIdx.x;
  const GOutT gox = (GOutT) static_cast<T *>(sg.ox), goy = (GOutT) static_cast<T *>(sg.oy), goz = (GOutT) static_cast<T *>(sg.oz);
  if ((int)blockIdx.x < dst_blocks) {  // (uniform) dst's own points, as stored
    const int i = blockIdx.x * kPointMergeThreads + tid;
    if (i >= sg.n_dst) return;
    const GPtr<T> gz = (GPtr<T>)static_cast<const T *>(sg.z);
    gox[i] = ((GPtr<T>)static_cast<const T *>(sg.x))[i];
    goy[i] = ((GPtr<T>)static_cast<const T *>(sg.y))[i];
    goz[i] = gz[i];
    if (sg.out_weighted) goz[sg.w_out + i] = sg.dst_weighted ? gz[sg.w_dst + i] : (T)1;
    return;
  }
  const int block = (int)blockIdx.x - dst_blocks;
  const int n = sg.n_src;
  const int first = block * kPointMergeThreads;
  if (first >= n) return;  // (uniform)
  const int i = first + tid;
  bool flag = false;
  T r[3];
  if (i < n) flag = point_merge_fate<T>(sg, i, need_pixel, margin, max_dt, cell_px, r) == 0;
  const int lane = tid & 63, wave = tid >> 6;
  const unsigned long long m = __builtin_amdgcn_ballot_w64(flag);
  if (lane == 0) s_cnt[wave] = __popcll(m);
  __syncthreads();
  if (!flag) return;
  unsigned int ordinal = (unsigned int)sg.block_counts[block];
  for (int w = 0; w < wave; ++w) ordinal += (unsigned int)s_cnt[w];
  ordinal += (unsigned int)__popcll(m & ((1ull << lane) - 1ull));
  if (cap && ordinal >= cap) return;
  const size_t slot = (size_t)sg.n_dst + ordinal;
  gox[slot] = r[0]; goy[slot] = r[1]; goz[slot] = r[2];
  if (sg.out_weighted) {
    const double w = sg.src_weighted ? (double)((GPtr<T>)static_cast<const T *>(sg.sz))[sg.w_src + i] : 1.0;
    goz[sg.w_out + slot] = (T)merge_weight(w, weight_scale);
  }
}
#endif  // !EA_TU_VARIANT

// ------------------------------------------------------------------------------------------------
// launchers (declared in ea_launch.h, called from ea_capi.hip)

// A run-time value becomes a template argument through these three: f is a generic lambda that receives the value as a
// std::integral_constant (spelled decltype(V)::value inside it) or, for the element type, a TypeTag.  A value outside a
// dispatch_int list is refused: nothing is rounded to a neighbouring kernel.  Which combinations a kernel template is
// compiled for is stated once per launcher, by an `if constexpr` in front of its one hipLaunchKernelGGL.
template <typename T> struct TypeTag { typedef T type; };
template <typename F> static inline hipError_t dispatch_bool(int v, F &&f) { return v ? f(std::true_type{}) : f(std::false_type{}); }
template <int... Vs, typename F> static inline hipError_t dispatch_int(int v, F &&f) {
  hipError_t e = hipErrorInvalidValue;
  (void)((v == Vs ? (e = f(std::integral_constant<int, Vs>{}), true) : false) || ...);
  return e;
}
template <typename F> static inline hipError_t dispatch_dtype(int dtype, F &&f) {
  return dtype == 1 ? f(TypeTag<float>{}) : f(TypeTag<double>{});
}

// grid, the packed `shape` word, the LDS tile and the dynamic LDS size of a launch of the fused family: `chunks` workgroups
// per term in x (rounded to the 8 XCDs under xcd_remap), one term per y
struct FusedGrid { dim3 grid; int chunks_per_xcd, shape, lds_texels; size_t shmem; };
static hipError_t fused_grid(const EvalLaunch &s, int nterms, int chunks, FusedGrid *g) {
  if (s.chunk <= 0 || s.chunk > 0xffff) return hipErrorInvalidValue;  // (NT * PPT <= 4096)
  g->chunks_per_xcd = (chunks + 7) / 8;
  g->grid = dim3(s.xcd_remap ? g->chunks_per_xcd * 8 : chunks, nterms);
  g->shape = s.chunk | ((s.xcd_remap ? 1 : 0) << 16) | ((s.terms_are_groups ? 1 : 0) << 17);
  const int esz = s.dtype == 1 ? 4 : 8;
  g->lds_texels = s.lds_bytes > 0 ? s.lds_bytes / esz : 0;
  g->shmem = (size_t)kHdrBytes + (size_t)g->lds_texels * esz;
  return hipSuccess;
}

// The launch shapes the evaluation kernels are compiled for, shared by the fused, fold and iteration launchers: fp32 takes
// 1, 2 or 4 points per lane at either workgroup size; fp64 (over either image type) has no PPT = 4 and runs 1024-thread
// workgroups at one point per lane only (128-VGPR budget)
template <typename T, int PPT, int NT> constexpr bool shape_exists() {
  return sizeof(T) == 4 || PPT == 1 || (PPT == 2 && NT == 256);
}

// The fused evaluation lives in two translation units: this file as it is (plain functor, every launch shape) and the
// same file compiled with -DEA_TU_VARIANT through ea_kernels_var.hip (the distortion / second-camera functors only).
// They differ in ONE compiler setting: the plain kernels are scheduled for instruction-level parallelism
// (-mllvm -amdgpu-sched-strategy=max-ilp: -2 .. -4 % kernel time), which costs the variant kernels a wave of occupancy in
// fp64 (123 -> 136 VGPRs) and 4-7 % of their time -- they keep the default strategy (build.py; profiles/LOG.md section 5b).
// kVarTU decides which half a translation unit compiles: fused_exists() below, and the #ifdef around the launchers.
#ifdef EA_TU_VARIANT
constexpr bool kVarTU = true;
#else
constexpr bool kVarTU = false;
#endif
// MODE 0: stencil rows from L2, 1: the footprint staged through LDS (flat addressing only), 2: fp32 with fp64 sums from the
// lane's sum on (no staging).  The fp32 mirror (IMG32) is fp64 arithmetic on the L2 path.  The variant functors: 256-thread
// workgroups, L2 path, 1-2 points per lane.
template <typename T, int PPT, int MODE, int NT, bool VAR, bool BUF, bool IMG32> constexpr bool fused_exists() {
  if (VAR != kVarTU || !shape_exists<T, PPT, NT>()) return false;
  if (VAR) return NT == 256 && PPT <= 2 && MODE == 0 && !IMG32;
  if (IMG32) return sizeof(T) == 8 && MODE == 0;
  return MODE == 0 || (MODE == 1 && !BUF) || (MODE == 2 && sizeof(T) == 4);
}

// tag 0: ea_eval_fused_kernel, tag 1: the same kernel under the name ea_eval_poses_grid_kernel (the pose-batched launches of the
// batches ea_eval_poses_kernel does not cover)
static hipError_t launch_fused_family(int tag, const EvalLaunch &s, const ProblemDesc *probs, int nterms, const PoseState *poses,
                                      double *partials, hipStream_t stream) {
  if (nterms <= 0 || s.max_chunks <= 0) return hipSuccess;
  FusedGrid g;
  if (hipError_t e = fused_grid(s, nterms, s.max_chunks, &g)) return e;
  const int mode = g.lds_texels > 0 ? 1 : s.wide ? 2 : 0;
  return dispatch_bool(tag, [&](auto TAG) { return dispatch_dtype(s.dtype, [&](auto TT) {
    return dispatch_int<1, 2, 4>(s.ppt, [&](auto PPT) { return dispatch_int<256, 1024>(s.nt, [&](auto NT) {
      return dispatch_int<0, 1, 2>(mode, [&](auto MODE) { return dispatch_bool(s.buffer_loads && mode != 1, [&](auto BUF) {
        return dispatch_bool(s.img32, [&](auto IMG32) {
          typedef typename decltype(TT)::type T;
          constexpr int P = decltype(PPT)::value, M = decltype(MODE)::value, N = decltype(NT)::value;
          constexpr bool B = decltype(BUF)::value, I = decltype(IMG32)::value;
          if constexpr (!fused_exists<T, P, M, N, kVarTU, B, I>()) return hipErrorInvalidValue;
          else {
            auto kernel = decltype(TAG)::value ? &ea_eval_poses_grid_kernel<T, P, M, N, kVarTU, B, I>
                                               : &ea_eval_fused_kernel<T, P, M, N, kVarTU, B, I>;
#ifdef EA_TU_VARIANT
            if (s.weighted)
              kernel = decltype(TAG)::value ? &ea_eval_poses_grid_w_kernel<T, P, M, N, kVarTU, B, I>
                                            : &ea_eval_fused_w_kernel<T, P, M, N, kVarTU, B, I>;
#else
            if (s.weighted) return hipErrorInvalidValue;  // (weighted terms are variants: ea_kernels_var.hip)
#endif
            hipLaunchKernelGGL(kernel, g.grid, dim3(N), g.shmem, stream, s.x0, s.y0, s.z0, s.n0, g.shape, g.chunks_per_xcd, probs,
                               poses, partials, g.lds_texels);
            return hipGetLastError();
          }
        }); }); });
    }); }); }); });
}

#ifdef EA_TU_VARIANT
hipError_t launch_eval_fused_var(int tag, const EvalLaunch &s, const ProblemDesc *probs, int nterms, const PoseState *poses,
                                 double *partials, hipStream_t stream) {
  return launch_fused_family(tag, s, probs, nterms, poses, partials, stream);
}
#else
hipError_t launch_eval_fused(const EvalLaunch &s, const ProblemDesc *probs, int nterms, const PoseState *poses, double *partials,
                             hipStream_t stream) {
  return s.variant ? launch_eval_fused_var(0, s, probs, nterms, poses, partials, stream)
                   : launch_fused_family(0, s, probs, nterms, poses, partials, stream);
}
hipError_t launch_eval_poses_grid(const EvalLaunch &s, const ProblemDesc *probs, int nterms, const PoseState *poses, double *partials,
                                  hipStream_t stream) {
  return s.variant ? launch_eval_fused_var(1, s, probs, nterms, poses, partials, stream)
                   : launch_fused_family(1, s, probs, nterms, poses, partials, stream);
}

// the wave-exchange instantiations (MODE = kModeExchange) of ea_eval_poses_kernel / ea_eval_starts_kernel: fp64 in 256-lane
// workgroups, at every shape the plain ones have
template <typename T, int NT> constexpr bool exchange_exists() { return sizeof(T) == 8 && NT == 256; }
// launch(MODE as a std::integral_constant, dynamic LDS bytes) with the reduction `exchange` asks for
template <typename T, int NT, typename F> static inline hipError_t launch_plain_or_exchange(int exchange, F &&launch) {
  if (!exchange) return launch(std::integral_constant<int, 0>{}, (size_t)kHdrBytes);
  if constexpr (!exchange_exists<T, NT>()) return hipErrorInvalidValue;
  else return launch(std::integral_constant<int, kModeExchange>{}, (size_t)kXchgBytes);
}
// what the flat launches (ea_poses_map.h) ask of a batch: plain functor, L2 path, one term per problem, whole chunks per
// workgroup, and a row index pose * rows + row that fits
static inline bool flat_launch_ok(const EvalLaunch &s, const PosesLaunch &p, int min_rows) {
  if (s.variant || s.lds_bytes > 0 || s.wide || !s.terms_are_groups || s.chunk != s.nt * s.ppt) return false;
  return p.g > 0 && p.rows >= min_rows && (int64_t)p.rows * p.g <= (int64_t)1 << 28;
}

// ea_eval_poses_kernel: g poses of a batch of `rows` partial rows per pose in one launch, `fold` (fold.n riders, 0 = none)
// riding in front (ea_poses_map.h).  Plain functor, L2 path, one term per problem.  p.exchange asks for the wave-exchange
// reduction (fp64 in 256-lane workgroups; refused elsewhere); the launch then takes kXchgBytes of dynamic LDS.
hipError_t launch_eval_poses(const EvalLaunch &s, const PosesLaunch &p, const ProblemDesc *probs, const PoseState *poses,
                             double *partials, const PosesFold &fold, hipStream_t stream) {
  if (!flat_launch_ok(s, p, 1) || fold.n < 0) return hipErrorInvalidValue;
  const int shape = poses_shape(s.xcd_remap != 0, p.order, p.single != 0, fold.n);
  const dim3 grid(poses_grid(p.rows, p.g, fold.n));
  return dispatch_dtype(s.dtype, [&](auto TT) { return dispatch_int<1, 2, 4>(s.ppt, [&](auto PPT) {
    return dispatch_int<256, 1024>(s.nt, [&](auto NT) { return dispatch_bool(s.buffer_loads, [&](auto BUF) {
      return dispatch_bool(s.img32, [&](auto IMG32) {
        typedef typename decltype(TT)::type T;
        constexpr int P = decltype(PPT)::value, N = decltype(NT)::value;
        constexpr bool B = decltype(BUF)::value, I = decltype(IMG32)::value;
        if constexpr (!fused_exists<T, P, 0, N, false, B, I>()) return hipErrorInvalidValue;
        else return launch_plain_or_exchange<T, N>(p.exchange, [&](auto MODE, size_t shmem) {
          hipLaunchKernelGGL((ea_eval_poses_kernel<T, P, decltype(MODE)::value, N, false, B, I>), grid, dim3(N), shmem, stream, s.x0,
                             s.y0, s.z0, s.n0, shape, p.g, p.rows, probs, poses, partials, fold);
          return hipGetLastError();
        });
      }); }); });
  }); });
}

// ea_eval_poses_lanes_kernel: the same launch with one pose per lane -- fp64 at the pose path's 256 x 2 shape only (the
// row is that shape's 512-point chunk); everything else is refused
hipError_t launch_eval_poses_lanes(const EvalLaunch &s, const PosesLaunch &p, const ProblemDesc *probs, const PoseState *poses,
                                   double *rows, const PosesTickets &tickets, hipStream_t stream) {
  if (!flat_launch_ok(s, p, 1) || s.dtype != EA_F64 || s.nt != 64 * kLanesWaves || s.ppt != 2) return hipErrorInvalidValue;
  if (tickets.on) {
    if (!tickets.partials || !tickets.counters || !tickets.out || !tickets.flags || tickets.count < 1) return hipErrorInvalidValue;
    // every counter of the launch starts at zero, whatever an earlier launch left (a call that failed half way included)
    const hipError_t e = hipMemsetAsync(tickets.counters, 0, poses_lanes_counters(poses_lanes_groups(p.g), p.rows, tickets.count) * sizeof(unsigned int), stream);
    if (e != hipSuccess) return e;
  }
  const int shape = poses_shape(s.xcd_remap != 0, p.order, p.single != 0, 0);
  const dim3 grid(poses_lanes_grid(p.rows, p.g, 0));
  return dispatch_bool(s.buffer_loads, [&](auto BUF) { return dispatch_bool(s.img32, [&](auto IMG32) {
    hipLaunchKernelGGL((ea_eval_poses_lanes_kernel<decltype(BUF)::value, decltype(IMG32)::value>), grid, dim3(64 * kLanesWaves), 0,
                       stream, shape, p.g, p.rows, probs, poses, rows, tickets);
    return hipGetLastError();
  }); });
}

// the fold that closes a call: fold.n results in workgroups of nt threads, the riders' summation order
hipError_t launch_poses_fold(int nt, const PosesFold &fold, hipStream_t stream) {
  if (fold.n <= 0) return hipErrorInvalidValue;  // (somebody has to raise the flag)
  if (nt == 1024) hipLaunchKernelGGL(ea_poses_fold_kernel<1024>, dim3(fold.n), dim3(1024), 0, stream, fold);
  else hipLaunchKernelGGL(ea_poses_fold_kernel<256>, dim3(fold.n), dim3(256), 0, stream, fold);
  return hipGetLastError();
}

// ea_cost_poses_kernel: launch_eval_poses' launch shape without riders, one narrow partial per workgroup.  Compiled for
// 256-lane workgroups in the shapes the evaluation kernels have; the fp32 mirror under fp64 arithmetic only.
template <typename T, int PPT, int NT, bool IMG32> constexpr bool cost_exists() {
  return NT == 256 && shape_exists<T, PPT, NT>() && (!IMG32 || sizeof(T) == 8);
}
hipError_t launch_cost_poses(const EvalLaunch &s, const PosesLaunch &p, const ProblemDesc *probs, const PoseState *poses,
                             void *partials, hipStream_t stream) {
  if (!flat_launch_ok(s, p, 1)) return hipErrorInvalidValue;
  const int shape = poses_shape(s.xcd_remap != 0, p.order, p.single != 0, 0);
  const dim3 grid(poses_grid(p.rows, p.g, 0));
  return dispatch_dtype(s.dtype, [&](auto TT) { return dispatch_int<1, 2, 4>(s.ppt, [&](auto PPT) {
    return dispatch_int<256>(s.nt, [&](auto NT) { return dispatch_bool(s.buffer_loads, [&](auto BUF) {
      return dispatch_bool(s.img32, [&](auto IMG32) {
        typedef typename decltype(TT)::type T;
        constexpr int P = decltype(PPT)::value, N = decltype(NT)::value;
        constexpr bool B = decltype(BUF)::value, I = decltype(IMG32)::value;
        if constexpr (!cost_exists<T, P, N, I>()) return hipErrorInvalidValue;
        else {
          hipLaunchKernelGGL((ea_cost_poses_kernel<T, P, N, B, I>), grid, dim3(N), 0, stream, s.x0, s.y0, s.z0, s.n0, shape, p.g,
                             p.rows, probs, poses, static_cast<CostPartial *>(partials));
          return hipGetLastError();
        }
      }); }); });
  }); });
}

// the fold behind a cost-only launch: fold.n results, fold.rows = the launch's narrow partials
hipError_t launch_cost_fold(const PosesFold &fold, hipStream_t stream) {
  if (fold.n <= 0) return hipErrorInvalidValue;  // (somebody has to raise the flag)
  hipLaunchKernelGGL(ea_cost_fold_kernel<256>, dim3(fold.n), dim3(256), 0, stream, fold);
  return hipGetLastError();
}

// ea_eval_starts_kernel: ea_eval_poses_kernel's launch of p.g poses over the piece [off, off + p.g) of a live list
hipError_t launch_eval_starts(const EvalLaunch &s, const PosesLaunch &p, const ProblemDesc *probs, const PoseState *poses,
                              double *partials, const int *live, const int *n_live, int off, hipStream_t stream) {
  if (!flat_launch_ok(s, p, 0) || s.nt != kLmThreads || off < 0) return hipErrorInvalidValue;
  if (p.rows == 0) return hipSuccess;  // not a single point in the batch
  const int shape = poses_shape(s.xcd_remap != 0, p.order, p.single != 0, 0);
  const dim3 grid(poses_grid(p.rows, p.g, 0));
  return dispatch_dtype(s.dtype, [&](auto TT) { return dispatch_int<1, 2, 4>(s.ppt, [&](auto PPT) {
    return dispatch_bool(s.buffer_loads, [&](auto BUF) { return dispatch_bool(s.img32, [&](auto IMG32) {
      typedef typename decltype(TT)::type T;
      constexpr int P = decltype(PPT)::value;
      constexpr bool B = decltype(BUF)::value, I = decltype(IMG32)::value;
      if constexpr (!fused_exists<T, P, 0, kLmThreads, false, B, I>()) return hipErrorInvalidValue;
      else return launch_plain_or_exchange<T, kLmThreads>(p.exchange, [&](auto MODE, size_t shmem) {
        hipLaunchKernelGGL((ea_eval_starts_kernel<T, P, decltype(MODE)::value, kLmThreads, false, B, I>), grid, dim3(kLmThreads), shmem,
                           stream, s.x0, s.y0, s.z0, s.n0, shape, p.g, p.rows, probs, poses, partials, live, n_live, off);
        return hipGetLastError();
      });
    }); });
  }); });
}

hipError_t launch_lm_step_starts(int g, const StartsStep &a, const LMOptions &lo, int side, hipStream_t stream) {
  if (g <= 0 || a.count <= 0 || (int64_t)g * a.count > kMaxStartSlots) return hipErrorInvalidValue;
  return dispatch_bool(lo.strategy != 0, [&](auto STRAT) { return dispatch_bool(side, [&](auto SIDE) {
    hipLaunchKernelGGL((ea_lm_step_starts_kernel<decltype(STRAT)::value ? 1 : 0, decltype(SIDE)::value>), dim3(starts_step_grid(g, a.count)),
                       dim3(kLmThreads), 0, stream, a, lo);
    return hipGetLastError();
  }); });
}

// evaluation into `partials` + the fold of fold.prev_rows -> fold.prev_out in one launch (ea_eval_fold_kernel): plain
// single-family problems on the L2 path
hipError_t launch_eval_fold(const EvalLaunch &s, const ProblemDesc *probs, int nterms, const PoseState *poses, double *partials,
                            const RidingFold &fold, hipStream_t stream) {
  if (s.variant || s.lds_bytes > 0 || s.wide || !s.terms_are_groups) return hipErrorInvalidValue;
  // a batch without a single point has nothing to evaluate, but the previous step's fold is still owed (its result slot
  // must not keep what an earlier owner of the memory left there): the stand-alone fold in the riders' summation order
  if (nterms > 0 && s.max_chunks <= 0) return launch_reduce_nt(s.nt, fold.groups, nterms, fold.prev_rows, fold.prev_out, stream);
  if (nterms <= 0) return hipSuccess;
  FusedGrid g;
  if (hipError_t e = fused_grid(s, nterms, s.max_chunks, &g)) return e;
  const dim3 grid_f(g.grid.x + 1, g.grid.y);  // (the fold workgroup: behind the evaluation's, after the rounding to the XCDs)
  return dispatch_dtype(s.dtype, [&](auto TT) { return dispatch_int<1, 2, 4>(s.ppt, [&](auto PPT) {
    return dispatch_int<256, 1024>(s.nt, [&](auto NT) { return dispatch_bool(s.buffer_loads, [&](auto BUF) {
      return dispatch_bool(s.img32, [&](auto IMG32) {
        typedef typename decltype(TT)::type T;
        constexpr int P = decltype(PPT)::value, N = decltype(NT)::value;
        constexpr bool I = decltype(IMG32)::value;
        if constexpr (!shape_exists<T, P, N>() || (I && sizeof(T) != 8)) return hipErrorInvalidValue;
        else {
          hipLaunchKernelGGL((ea_eval_fold_kernel<T, P, N, decltype(BUF)::value, I>), grid_f, dim3(N), g.shmem, stream, s.x0, s.y0,
                             s.z0, s.n0, g.shape, g.chunks_per_xcd, probs, poses, partials, g.lds_texels, fold.groups,
                             fold.prev_rows, fold.prev_out);
          return hipGetLastError();
        }
      }); }); });
  }); });
}

// the stand-alone fold in the order the riding folds of an nt-thread evaluation use
hipError_t launch_reduce_nt(int nt, const GroupDesc *groups, int count, const double *partials, EvalOut *out,
                            hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  if (nt == 1024) hipLaunchKernelGGL(ea_reduce_kernel, dim3(count), dim3(kFoldThreads), 0, stream, groups, partials, out);
  else hipLaunchKernelGGL(ea_reduce256_kernel, dim3(count), dim3(kLmThreads), 0, stream, groups, partials, out);
  return hipGetLastError();
}

hipError_t launch_eval_points(int dtype, const ProblemDesc *probs, int problem, int n, const PoseState *poses,
                              double *r_out, double *J_out, int corrected, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  const int grid = (n + kBlockThreads - 1) / kBlockThreads;
  return dispatch_dtype(dtype, [&](auto TT) {
    hipLaunchKernelGGL((ea_eval_points_kernel<typename decltype(TT)::type>), dim3(grid), dim3(kBlockThreads), 0, stream, probs,
                       problem, poses, r_out, J_out, corrected);
    return hipGetLastError();
  });
}

// materialised mode: rows of every term of the batch into the caller's device arrays (ea_eval_rows_kernel).  The distortion /
// second-camera terms address flat; the column-major layout has no staged form; the fp32 mirror is fp64 over plain terms.
hipError_t launch_eval_rows(const RowsLaunch &s, const ProblemDesc *probs, int nterms, const PoseState *poses, void *r_out,
                            void *J_out, unsigned int *n_invalid, hipStream_t stream) {
  if (nterms <= 0 || s.max_n <= 0) return hipSuccess;
  const int chunks = (int)((s.max_n + kBlockThreads - 1) / kBlockThreads);
  const int chunks_per_xcd = (chunks + 7) / 8;
  const dim3 grid(chunks_per_xcd * 8, nterms);
  return dispatch_dtype(s.dtype, [&](auto TT) { return dispatch_bool(s.variant, [&](auto VAR) {
    return dispatch_bool(s.buffer_loads && !s.variant, [&](auto BUF) { return dispatch_int<0, 1>(s.layout, [&](auto LAYOUT) {
      return dispatch_bool(s.staged && s.layout == 0, [&](auto STAGED) { return dispatch_bool(s.img32, [&](auto IMG32) {
        typedef typename decltype(TT)::type T;
        constexpr bool V = decltype(VAR)::value, B = decltype(BUF)::value, S = decltype(STAGED)::value, I = decltype(IMG32)::value;
        constexpr int L = decltype(LAYOUT)::value;
        if constexpr ((V && B) || (L == 1 && S) || (I && (sizeof(T) != 8 || V))) return hipErrorInvalidValue;
        else {
          hipLaunchKernelGGL((ea_eval_rows_kernel<T, V, B, L, S, I>), grid, dim3(kBlockThreads), 0, stream, probs, poses,
                             chunks_per_xcd, s.corrected, s.nontemporal, s.total_rows, static_cast<T *>(r_out),
                             static_cast<T *>(J_out), n_invalid);
          return hipGetLastError();
        }
      }); }); });
    }); }); });
}

hipError_t launch_pixel_cost(int dtype, const ProblemDesc *probs, int problem, int n, const PoseState *poses, void *partials,
                             hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  const int grid = (n + kBlockThreads - 1) / kBlockThreads;
  return dispatch_dtype(dtype, [&](auto TT) {
    hipLaunchKernelGGL((ea_pixel_cost_kernel<typename decltype(TT)::type>), dim3(grid), dim3(kBlockThreads), 0, stream, probs,
                       problem, poses, static_cast<PixelCostPartial *>(partials));
    return hipGetLastError();
  });
}

hipError_t launch_reduce(const GroupDesc *groups, int count, const double *partials, EvalOut *out,
                         hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  hipLaunchKernelGGL(ea_reduce_kernel, dim3(count), dim3(kFoldThreads), 0, stream, groups, partials, out);
  return hipGetLastError();
}

hipError_t launch_reduce_done(const GroupDesc *groups, int count, const double *partials, EvalOut *out, unsigned int *counter,
                              int *host_flag, int seq, hipStream_t stream) {
  if (count <= 0) return hipErrorInvalidValue;  // (somebody has to raise the flag)
  hipLaunchKernelGGL(ea_reduce_done_kernel, dim3(count), dim3(kFoldThreads), 0, stream, groups, partials, out, counter, host_flag, seq);
  return hipGetLastError();
}

hipError_t launch_lm_step(const GroupDesc *groups, int count, const double *partials, const LMLaunch &lm, hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  return dispatch_bool(lm.opt->strategy != 0, [&](auto STRAT) { return dispatch_bool(lm.side, [&](auto SIDE) {
    hipLaunchKernelGGL((ea_lm_step_kernel<decltype(STRAT)::value ? 1 : 0, decltype(SIDE)::value>), dim3(count), dim3(kLmThreads), 0,
                       stream, groups, partials, lm.poses, lm.states, lm.cold, lm.traces, *lm.opt, lm.progress, lm.host_states,
                       lm.host_traces, lm.first, lm.post_done);
    return hipGetLastError();
  }); });
}

// ea_lm_iter_kernel: launch j of a solve reads what launch j - 1 wrote (state, cold system, rows) and writes the other
// buffer of each pair.  One plain residual family per problem in 256-thread workgroups on the L2 path; no fp32 x IMG32.
hipError_t launch_lm_iter(const EvalLaunch &s, const ProblemDesc *probs, int count, const GroupDesc *groups, const LMLaunch &lm,
                          const LMIterPairs &io, hipStream_t stream) {
  if (count <= 0) return hipSuccess;
  if (s.variant || s.lds_bytes > 0 || s.wide || !s.terms_are_groups || s.nt != kLmThreads || s.chunk != kLmThreads * s.ppt)
    return hipErrorInvalidValue;
  FusedGrid g;
  // the grid is one workgroup wider than the evaluation's (the writer), THEN rounded to the 8 XCDs
  if (hipError_t e = fused_grid(s, count, s.max_chunks + 1, &g)) return e;
  return dispatch_dtype(s.dtype, [&](auto TT) { return dispatch_int<1, 2, 4>(s.ppt, [&](auto PPT) {
    return dispatch_bool(s.buffer_loads, [&](auto BUF) { return dispatch_bool(s.img32, [&](auto IMG32) {
      return dispatch_bool(lm.opt->strategy != 0, [&](auto STRAT) { return dispatch_bool(lm.side, [&](auto SIDE) {
        typedef typename decltype(TT)::type T;
        constexpr int P = decltype(PPT)::value;
        constexpr bool I = decltype(IMG32)::value;
        if constexpr (!shape_exists<T, P, kLmThreads>() || (I && sizeof(T) != 8)) return hipErrorInvalidValue;
        else {
          hipLaunchKernelGGL((ea_lm_iter_kernel<T, P, decltype(BUF)::value, I, decltype(STRAT)::value ? 1 : 0, decltype(SIDE)::value>),
                             g.grid, dim3(kLmThreads), g.shmem, stream, s.x0, s.y0, s.z0, s.n0, g.shape, g.chunks_per_xcd, io.rows_in,
                             lm.first.tile_begin, lm.first.tile_end, probs, lm.poses, io.rows_out, groups, io.st_in, io.st_out,
                             io.cold_in, io.cold_out, lm.traces, *lm.opt, lm.progress, lm.host_states, lm.host_traces, lm.post_done);
          return hipGetLastError();
        }
      }); }); });
    }); }); });
}

#ifdef EA_STAMPS
hipError_t set_stamp_buffer(unsigned long long *buf) { return hipMemcpyToSymbol(HIP_SYMBOL(g_stamp_buf), &buf, sizeof(buf)); }
hipError_t set_lm_stamp_buffer(unsigned long long *buf) { return hipMemcpyToSymbol(HIP_SYMBOL(g_lm_stamp_buf), &buf, sizeof(buf)); }
#endif

hipError_t launch_selftest_reduce(const float *in, float *a, float *b, float *c, float *d, double *o32, double *o64,
                                  hipStream_t stream) {
  hipLaunchKernelGGL(ea_selftest_reduce_kernel, dim3(1), dim3(64), 0, stream, in, a, b, c, d, o32, o64);
  return hipGetLastError();
}

__global__ void ea_empty_kernel() {}
hipError_t launch_empty(int grid, int block, hipStream_t stream) {
  hipLaunchKernelGGL(ea_empty_kernel, dim3(grid), dim3(block), 0, stream);
  return hipGetLastError();
}

hipError_t launch_make_poses(const double *qt, int n, int count, const ProblemDesc *probs, const GroupDesc *groups,
                             PoseState *out, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(ea_make_poses_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, qt, n, count, probs, groups, out);
  return hipGetLastError();
}

hipError_t launch_pad_image(int dtype, const void *src, int H, int W, void *dst, int pitch, float *dst32, int *inexact,
                            hipStream_t stream) {
  dim3 block(256), grid((W + 2 * kImagePad + 255) / 256, H + 2 * kImagePad);
  if (dtype == 1)
    hipLaunchKernelGGL((ea_pad_image_kernel<float>), grid, block, 0, stream, (const float *)src, H, W, (float *)dst, pitch, nullptr, nullptr);
  else
    hipLaunchKernelGGL((ea_pad_image_kernel<double>), grid, block, 0, stream, (const double *)src, H, W, (double *)dst, pitch, dst32, inexact);
  return hipGetLastError();
}

hipError_t launch_aos_to_soa(int dtype, const double *src, long long n, int stride, void *x, void *y, void *z, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  const dim3 grid((unsigned)((n + 255) / 256));
  if (dtype == 1) hipLaunchKernelGGL((ea_aos_to_soa_kernel<float>), grid, dim3(256), 0, stream, src, n, stride, (float *)x, (float *)y, (float *)z);
  else hipLaunchKernelGGL((ea_aos_to_soa_kernel<double>), grid, dim3(256), 0, stream, src, n, stride, (double *)x, (double *)y, (double *)z);
  return hipGetLastError();
}

hipError_t launch_store_weights(int dtype, int src_is_double, const void *src, const int32_t *order, long long n, void *dst,
                                hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  const dim3 grid((unsigned)((n + 255) / 256));
  if (dtype == 1 && src_is_double)
    hipLaunchKernelGGL((ea_store_weights_kernel<double, float>), grid, dim3(256), 0, stream, (const double *)src, order, n, (float *)dst);
  else if (dtype == 1)
    hipLaunchKernelGGL((ea_store_weights_kernel<float, float>), grid, dim3(256), 0, stream, (const float *)src, order, n, (float *)dst);
  else
    hipLaunchKernelGGL((ea_store_weights_kernel<double, double>), grid, dim3(256), 0, stream, (const double *)src, order, n, (double *)dst);
  return hipGetLastError();
}

hipError_t launch_depth_weights(int dtype, const void *z, long long n, double z_ref, int power, void *w, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  const dim3 grid((unsigned)((n + 255) / 256));
  if (dtype == 1) hipLaunchKernelGGL((ea_depth_weights_kernel<float>), grid, dim3(256), 0, stream, (const float *)z, n, z_ref, power, (float *)w);
  else hipLaunchKernelGGL((ea_depth_weights_kernel<double>), grid, dim3(256), 0, stream, (const double *)z, n, z_ref, power, (double *)w);
  return hipGetLastError();
}

hipError_t launch_depth_weights_frames(int dtype, const FramesLaunch &f, long long max_n, hipStream_t stream) {
  if (max_n <= 0) return hipSuccess;
  if (f.n < 1 || f.n > 65535 || !f.slots) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((max_n + 255) / 256), 1, (unsigned)f.n);
  if (dtype == 1) hipLaunchKernelGGL((ea_depth_weights_frames_kernel<float>), grid, dim3(256), 0, stream, f.slots);
  else hipLaunchKernelGGL((ea_depth_weights_frames_kernel<double>), grid, dim3(256), 0, stream, f.slots);
  return hipGetLastError();
}

// the select kernels' launches: x = chunks of the longest segment, y = segments
static hipError_t select_grid(const SelectWork &w, int per_workgroup, dim3 *grid) {
  if (w.nseg < 1 || w.nseg > 65535 || w.nq < 1 || w.nq > kSelectMaxQ || w.max_n < 0) return hipErrorInvalidValue;
  const int64_t chunks = ((int64_t)w.max_n + per_workgroup - 1) / per_workgroup;
  *grid = dim3((unsigned)(chunks > 0 ? chunks : 1), (unsigned)w.nseg);
  return hipSuccess;
}
hipError_t launch_select_clear(const SelectWork &w, hipStream_t stream) {
  // (n_valid and the histograms are one range: SelectWork)
  return hipMemsetAsync(w.n_valid, 0, w.clear_bytes, stream);
}
hipError_t launch_select_keys(int dtype, const SelectWork &w, const ProblemDesc *probs, const PoseState *poses, hipStream_t stream) {
  dim3 grid;
  if (hipError_t e = select_grid(w, kSelectThreads, &grid)) return e;
  if (w.max_n == 0) return hipSuccess;
  if (dtype == 1) hipLaunchKernelGGL((ea_select_keys_kernel<float>), grid, dim3(kSelectThreads), 0, stream, probs, w.segs, poses, w.keys);
  else hipLaunchKernelGGL((ea_select_keys_kernel<double>), grid, dim3(kSelectThreads), 0, stream, probs, w.segs, poses, w.keys);
  return hipGetLastError();
}
hipError_t launch_select_keys_values(const SelectWork &w, const double *values, hipStream_t stream) {
  dim3 grid;
  if (hipError_t e = select_grid(w, kSelectThreads, &grid)) return e;
  if (w.max_n == 0) return hipSuccess;
  hipLaunchKernelGGL(ea_select_keys_values_kernel, grid, dim3(kSelectThreads), 0, stream, values, w.segs, w.keys);
  return hipGetLastError();
}
hipError_t launch_select(const SelectWork &w, hipStream_t stream) {
  dim3 grid;
  if (hipError_t e = select_grid(w, kSelectChunk, &grid)) return e;
  for (int pass = 0; pass < kSelectPasses; ++pass) {
    if (w.max_n > 0) hipLaunchKernelGGL(ea_select_hist_kernel, grid, dim3(kSelectThreads), 0, stream, w.keys, w.segs, w.prefix, w.nq, pass, w.hist);
    hipLaunchKernelGGL(ea_select_scan_kernel, dim3((unsigned)w.nseg), dim3(kSelectThreads), 0, stream, w.probs, w.nq, pass, w.n_valid,
                       w.prefix, w.rank, w.hist, w.out_values, w.out_n_valid);
    if (hipError_t e = hipGetLastError()) return e;
  }
  return hipSuccess;
}

hipError_t launch_pose_stats(int dtype, const PoseStatsWork &w, const ProblemDesc *probs, const PoseState *poses, hipStream_t stream) {
  if (w.nseg < 1 || w.nseg > 65535 || w.max_n < 0 || w.margin < 0 || !w.segs || !w.partials || !w.out) return hipErrorInvalidValue;
  const dim3 grid((unsigned)pose_stats_rows(w.max_n), (unsigned)w.nseg);
  if (w.max_n > 0) {
    if (dtype == 1)
      hipLaunchKernelGGL((ea_pose_stats_kernel<float>), grid, dim3(kPoseStatsThreads), 0, stream, probs, w.segs, poses, w.margin,
                         w.inlier_residual, w.partials);
    else
      hipLaunchKernelGGL((ea_pose_stats_kernel<double>), grid, dim3(kPoseStatsThreads), 0, stream, probs, w.segs, poses, w.margin,
                         w.inlier_residual, w.partials);
  }
  hipLaunchKernelGGL(ea_pose_stats_fold_kernel, dim3((unsigned)w.nseg), dim3(64), 0, stream, w.segs, w.partials, w.out);
  return hipGetLastError();
}

hipError_t launch_reproject(int dtype, const ReprojectWork &w, const ProblemDesc *probs, hipStream_t stream) {
  if (w.nseg < 1 || w.nseg > 65535 || w.max_n < 0 || !w.segs || (w.paint ? !w.counts : !w.uv)) return hipErrorInvalidValue;
  if (w.max_n == 0) return hipSuccess;
  const dim3 grid((unsigned)((w.max_n + kReprojectThreads - 1) / kReprojectThreads), (unsigned)w.nseg);
  return dispatch_dtype(dtype, [&](auto TT) {
    return dispatch_bool(w.paint, [&](auto PAINT) {
      hipLaunchKernelGGL((ea_reproject_kernel<typename decltype(TT)::type, decltype(PAINT)::value>), grid, dim3(kReprojectThreads), 0,
                         stream, probs, w.segs, w.uv, w.color, w.counts);
      return hipGetLastError();
    });
  });
}

hipError_t launch_depth_gate(int dtype, const DepthGateWork &w, const ProblemDesc *probs, hipStream_t stream) {
  if (w.nseg < 1 || w.nseg > 65535 || w.max_n < 0 || !w.segs || !w.counts) return hipErrorInvalidValue;
  if (w.max_n == 0) return hipSuccess;
  const dim3 grid((unsigned)((w.max_n + kDepthGateThreads - 1) / kDepthGateThreads), (unsigned)w.nseg);
  return dispatch_dtype(dtype, [&](auto TT) {
    return dispatch_bool(w.kind == EA_DEPTH_F32, [&](auto F32) {
      return dispatch_int<0, 1, 2, 3>(w.radius, [&](auto RR) {
        typedef typename std::conditional<decltype(F32)::value, float, uint16_t>::type RAW;
        hipLaunchKernelGGL((ea_depth_gate_kernel<typename decltype(TT)::type, RAW, decltype(RR)::value>), grid,
                           dim3(kDepthGateThreads), 0, stream, probs, w.segs, w.rule, w.counts);
        return hipGetLastError();
      });
    });
  });
}

hipError_t launch_point_select(int dtype, const PointSelectWork &w, hipStream_t stream) {
  if (w.nseg < 1 || w.nseg > 65535 || w.max_n < 0 || !w.segs || !w.out || w.stride < 1 || (w.cell_px > 0 && !w.tables))
    return hipErrorInvalidValue;
  if (w.max_n == 0) return hipSuccess;
  const dim3 grid((unsigned)((w.max_n + kPointSelectThreads - 1) / kPointSelectThreads), (unsigned)w.nseg);
  if (w.cell_px > 0)
    if (hipError_t e = hipMemsetAsync(w.tables, 0xFF, w.table_bytes, stream)) return e;
  return dispatch_dtype(dtype, [&](auto TT) {
    typedef typename decltype(TT)::type T;
    if (w.cell_px > 0) {
      if (w.nearest)
        hipLaunchKernelGGL((ea_point_select_keys_kernel<T, 0>), grid, dim3(kPointSelectThreads), 0, stream, w.segs, w.cell_px, 1);
      hipLaunchKernelGGL((ea_point_select_keys_kernel<T, 1>), grid, dim3(kPointSelectThreads), 0, stream, w.segs, w.cell_px, w.nearest);
    }
    hipLaunchKernelGGL((ea_point_select_count_kernel<T>), grid, dim3(kPointSelectThreads), 0, stream, w.segs, w.cell_px, w.outside, w.out);
    hipLaunchKernelGGL(ea_point_select_scan_kernel, dim3((unsigned)w.nseg), dim3(kPointSelectScan), 0, stream, w.segs, w.out);
    hipLaunchKernelGGL((ea_point_select_compact_kernel<T>), grid, dim3(kPointSelectThreads), 0, stream, w.segs, w.cell_px, w.outside,
                       w.stride, w.target, w.out);
    return hipGetLastError();
  });
}

hipError_t launch_point_transform(int dtype, const PointTransformSeg *segs, int nseg, int max_n, hipStream_t stream) {
  if (nseg < 1 || nseg > 65535 || max_n < 0 || !segs) return hipErrorInvalidValue;
  if (max_n == 0) return hipSuccess;
  const dim3 grid((unsigned)((max_n + kPointMergeThreads - 1) / kPointMergeThreads), (unsigned)nseg);
  return dispatch_dtype(dtype, [&](auto TT) {
    hipLaunchKernelGGL((ea_point_transform_kernel<typename decltype(TT)::type>), grid, dim3(kPointMergeThreads), 0, stream, segs);
    return hipGetLastError();
  });
}

hipError_t launch_point_merge(int dtype, const PointMergeWork &w, hipStream_t stream) {
  if (w.nseg < 1 || w.nseg > 65535 || w.max_dst < 0 || w.max_src < 1 || !w.segs || !w.out || !w.scan_segs || !w.scan_out ||
      (w.cell_px > 0 && !w.tables))
    return hipErrorInvalidValue;
  const unsigned dst_blocks = (unsigned)((w.max_dst + kPointMergeThreads - 1) / kPointMergeThreads);
  const unsigned src_blocks = (unsigned)((w.max_src + kPointMergeThreads - 1) / kPointMergeThreads);
  const dim3 block(kPointMergeThreads), grid_dst(dst_blocks, (unsigned)w.nseg), grid_src(src_blocks, (unsigned)w.nseg);
  if (w.cell_px > 0)
    if (hipError_t e = hipMemsetAsync(w.tables, 0xFF, w.table_bytes, stream)) return e;
  return dispatch_dtype(dtype, [&](auto TT) {
    typedef typename decltype(TT)::type T;
    if (w.cell_px > 0) {
      if (dst_blocks) hipLaunchKernelGGL((ea_point_merge_occupancy_kernel<T>), grid_dst, block, 0, stream, w.segs, w.cell_px);
      if (w.nearest) hipLaunchKernelGGL((ea_point_merge_keys_kernel<T, 0>), grid_src, block, 0, stream, w.segs, w.margin, w.max_dt, w.cell_px, 1);
      hipLaunchKernelGGL((ea_point_merge_keys_kernel<T, 1>), grid_src, block, 0, stream, w.segs, w.margin, w.max_dt, w.cell_px, w.nearest);
    }
    hipLaunchKernelGGL((ea_point_merge_count_kernel<T>), grid_src, block, 0, stream, w.segs, w.need_pixel, w.margin, w.max_dt, w.cell_px, w.out);
    hipLaunchKernelGGL(ea_point_select_scan_kernel, dim3((unsigned)w.nseg), dim3(kPointSelectScan), 0, stream, w.scan_segs, w.scan_out);
    hipLaunchKernelGGL((ea_point_merge_copy_kernel<T>), dim3(dst_blocks + src_blocks, (unsigned)w.nseg), block, 0, stream, w.segs,
                       (int)dst_blocks, w.need_pixel, w.margin, w.max_dt, w.cell_px, w.cap, w.weight_scale);
    return hipGetLastError();
  });
}

hipError_t launch_grid_to_image(int dtype, const double *grid, int W, int H, void *dst, int pitch, float *dst32, int *inexact,
                                hipStream_t stream) {
  dim3 block(256), tiles((W + 2 * kImagePad + 31) / 32, (H + 2 * kImagePad + 31) / 32);
  if (dtype == 1) hipLaunchKernelGGL((ea_grid_to_image_kernel<float>), tiles, block, 0, stream, grid, W, H, (float *)dst, pitch, nullptr, nullptr);
  else hipLaunchKernelGGL((ea_grid_to_image_kernel<double>), tiles, block, 0, stream, grid, W, H, (double *)dst, pitch, dst32, inexact);
  return hipGetLastError();
}

#endif  // EA_TU_VARIANT

}  // namespace ea
