// ea_pair_log.h — the fp64 logarithm of the Cauchy loss (fused_chunk and cost_item, ea_kernels.hip), once per point and once
// per PAIR of points, as templates over the few machine operations they need, so that the host compiles the same text with
// stand-ins for the intrinsics and measures it without a device (tests/pair_log_host_shim.cpp).  Further down: once per RUN
// of points, for a lane that walks many (lanes_sums / lanes_run; tests/pair_log_run_host_shim.cpp).
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

// ---- the running product: one logarithm for a whole run of factors ---------------------------------------------------------
// A lane that walks many points (the pose-per-lane kernel: 128 per sub-run) needs sum_i log s_i = log prod_i s_i only.  The
// product is carried as P + L -- P the rounded product, L the accumulated rounding error (one fma per factor gives the exact
// error of P s, a second carries the old L along) -- times 2^E, and the logarithm is taken ONCE behind the run:
// log(P + L) = log P + L / P to second order in n 2^-53, the same correction pl_log_pair makes for its single product.
//
// The factors are s = 1 + x >= 1, so P stays >= 1 (>= 1/4 once renormalised) and cannot underflow; and no factor is split by
// frexp on the common path: a factor near 1 stays near 1 (mantissas in [0.5, 1) per factor would leave E ln 2 - log P to
// cancel, which costs 1e-4 relative at x ~ 1e-12).  Only when the rounded product p = P s passes 2^400 -- infinity included:
// p is thrown away then -- P and s are brought back to [0.5, 1), their exponents go to E and p is formed again.  So P <= 2^400
// before every step, whatever finite s arrives, and one comparison per factor guards the run.  From the first
// renormalisation on the sum is >= 400 ln 2 and log P >= log(1/4): nothing of that size cancels.
//
// E: a renormalisation adds at most 401 + 1024, so |E| < 128 * 1425 < 2^18 over the 128 factors of a sub-run -- exact as an
// int and as a double.  That is past the 2^11 up to which E * kLn2Hi is an exact product, and need not be inside: the
// recombination is fma(E, hi, fma(E, lo, .)), where each product is rounded together with its sum only, and hi + lo is ln 2
// to 2^-86 for any E.
constexpr double kRunBound = 0x1p400;

// p = P * s as rounded: does the step have to renormalise first?
template <class Ops> EA_HD inline bool pl_run_high(double p) { return p > Ops::sconst(kRunBound); }
// the slow path: P, L and s scaled down by the exponents of P and s, which go to E; returns the new P s
template <class Ops> EA_HD inline double pl_run_renorm(double &P, double &L, int &E, double &s) {
  const int eP = Ops::frexp_exp(P), es = Ops::frexp_exp(s);
  P = Ops::frexp_mant(P);
  L = Ops::ldexp(L, -eP);
  s = Ops::frexp_mant(s);
  E += eP + es;
  return P * s;
}
// (P + L) *= s with p = P * s
EA_HD inline void pl_run_take(double &P, double &L, double s, double p) {
  const double err = __builtin_fma(P, s, -p);  // P s = p + err exactly
  L = __builtin_fma(L, s, err);
  P = p;
}
// one factor, as a lane on its own takes it (the kernel makes the test wave-uniform first); true: it renormalised
template <class Ops> EA_HD inline bool pl_run_step(double &P, double &L, int &E, double s) {
  double p = P * s;
  const bool high = pl_run_high<Ops>(p);
  if (high) p = pl_run_renorm<Ops>(P, L, E, s);
  pl_run_take(P, L, s, p);
  return high;
}
// log((P + L) 2^E); P = 1, L = 0, E = 0 (no factor, or all of them 1) gives exactly 0
template <class Ops> EA_HD inline double pl_run_log(double P, double L, int E) {
  const double lg = __builtin_fma(L, Ops::rcp(P), pl_log<Ops>(P));
  const double ef = (double)E;
  return __builtin_fma(ef, Ops::sconst(kLn2Hi), __builtin_fma(ef, Ops::sconst(kLn2Lo), lg));
}

}  // namespace ea
