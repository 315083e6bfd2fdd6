// ea_pair_log.h — the fp64 logarithm of the Cauchy loss (fused_chunk and cost_item, ea_kernels.hip), once per point and once
// per PAIR of points, as templates over the few machine operations they need, so that the host compiles the same text with
// stand-ins for the intrinsics and measures it without a device (tests/pair_log_host_shim.cpp).
//
// The cost of a lane with two points needs log(s0) + log(s1) = log(s0 s1) only.  log_pair multiplies the two MANTISSAS (no
// input can overflow or underflow the product), keeps the rounding error of that product (one fma) and returns it to the
// result as err / p -- log(p + err) = log p + err / p to second order in 2^-53 -- so the pair agrees with the two separate
// logs to their own rounding.  The correction is what makes the form usable: the arguments are 1 + x with x down to 1e-15,
// where log(s0 s1) ~ x0 + x1 and half an ulp of the product (1.1e-16) is a RELATIVE error of 1.1e-16 / (x0 + x1).
//
// Ops supplies: frexp_mant (into [0.5, 1)), frexp_exp, ldexp, rcp (the raw reciprocal approximation, ~2^-26 or better) and
// sconst (the value itself; on the device through a scalar register, so that the series' coefficients are operands of
// v_fma_f64 and no pair of v_mov_b32 rebuilds each of them in vector registers per use).
#pragma once

#include "ea_types.h"

namespace ea {

constexpr double kSqrtHalf = 0.70710678118654752440;
// ln 2 split so that e * hi is exact for |e| < 2^11
constexpr double kLn2Hi = 0.693147180369123816490, kLn2Lo = 1.90821492927058770002e-10;

// raw reciprocal + two Newton steps: <= 1 ulp
template <class Ops> EA_HD inline double pl_rcp(double x) {
  double r = Ops::rcp(x);
  double e = __builtin_fma(-x, r, 1.0);
  r = __builtin_fma(r, e, r);
  e = __builtin_fma(-x, r, 1.0);
  return __builtin_fma(r, e, r);
}

// log m for m in [sqrt(1/2), sqrt(2)): 2 atanh z, z = (m - 1) / (m + 1), |z| <= 0.1716, as the odd series to z^21 (next term
// < 1e-18 relative)
template <class Ops> EA_HD inline double pl_log_mantissa(double m) {
  const double z = (m - 1.0) * pl_rcp<Ops>(m + 1.0);
  const double z2 = z * z;
  double p = 2.0 / 21.0;
  p = __builtin_fma(p, z2, Ops::sconst(2.0 / 19.0));
  p = __builtin_fma(p, z2, Ops::sconst(2.0 / 17.0));
  p = __builtin_fma(p, z2, Ops::sconst(2.0 / 15.0));
  p = __builtin_fma(p, z2, Ops::sconst(2.0 / 13.0));
  p = __builtin_fma(p, z2, Ops::sconst(2.0 / 11.0));
  p = __builtin_fma(p, z2, Ops::sconst(2.0 / 9.0));
  p = __builtin_fma(p, z2, Ops::sconst(2.0 / 7.0));
  p = __builtin_fma(p, z2, Ops::sconst(2.0 / 5.0));
  p = __builtin_fma(p, z2, Ops::sconst(2.0 / 3.0));
  return __builtin_fma(z * z2, p, z + z);
}

// log x, x > 0 finite: frexp to m in [sqrt(1/2), sqrt(2)), the series, e ln 2.  ~2 ulp.
template <class Ops> EA_HD inline double pl_log(double x) {
  double m = Ops::frexp_mant(x);  // [0.5, 1)
  int e = Ops::frexp_exp(x);
  const bool lo = m < Ops::sconst(kSqrtHalf);
  m = Ops::ldexp(m, lo ? 1 : 0);
  e -= lo ? 1 : 0;
  const double lm = pl_log_mantissa<Ops>(m);
  const double ef = (double)e;
  return __builtin_fma(ef, Ops::sconst(kLn2Hi), __builtin_fma(ef, Ops::sconst(kLn2Lo), lm));
}

// log s0 + log s1, both > 0 finite.  CORRECT = false is the form without the error term, kept for the host test that shows
// why it is there; the kernels use the default.
template <class Ops, bool CORRECT = true> EA_HD inline double pl_log_pair(double s0, double s1) {
  const double m0 = Ops::frexp_mant(s0), m1 = Ops::frexp_mant(s1);  // [0.5, 1) each
  int e = Ops::frexp_exp(s0) + Ops::frexp_exp(s1);
  const double p = m0 * m1;                       // [0.25, 1)
  const double err = __builtin_fma(m0, m1, -p);   // m0 m1 = p + err exactly
  double m = Ops::frexp_mant(p);
  e += Ops::frexp_exp(p);                         // 0 or -1
  const bool lo = m < Ops::sconst(kSqrtHalf);
  m = Ops::ldexp(m, lo ? 1 : 0);
  e -= lo ? 1 : 0;
  double lm = pl_log_mantissa<Ops>(m);
  if (CORRECT) lm = __builtin_fma(err, Ops::rcp(p), lm);
  const double ef = (double)e;
  return __builtin_fma(ef, Ops::sconst(kLn2Hi), __builtin_fma(ef, Ops::sconst(kLn2Lo), lm));
}

}  // namespace ea
