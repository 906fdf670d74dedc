// forest/gnx_det_exp.h — the deterministic float64 exp of the two tree trainers (k_train_gbt.hip, forest/k_train_gbt_base.hip).
//
// Both trainers are held bit-exact to restatements on the CPU (the oracle's gnxo_train_gbt, tests/gbt_base_exact.py), which must
// reproduce every probability: so exp is plain IEEE operations in a FIXED order — range reduction by rint and a two-part ln 2, a
// degree-13 Horner polynomial from the highest coefficient down, ldexp — and the library is built with -ffp-contract=off.  This is
// the one definition; the restatements follow it, operation by operation.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ double det_exp(double x) {  // x <= 0; the same operations, in the same order, as the oracle's
  if (!(x > -745.0)) return 0.0;
  const double LOG2E = 1.4426950408889634, LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10;
  const double kf = rint(x * LOG2E);
  const double r = (x - kf * LN2_HI) - kf * LN2_LO;
  double p = 1.0 / 6227020800.0;
  p = p * r + 1.0 / 479001600.0;
  p = p * r + 1.0 / 39916800.0;
  p = p * r + 1.0 / 3628800.0;
  p = p * r + 1.0 / 362880.0;
  p = p * r + 1.0 / 40320.0;
  p = p * r + 1.0 / 5040.0;
  p = p * r + 1.0 / 720.0;
  p = p * r + 1.0 / 120.0;
  p = p * r + 1.0 / 24.0;
  p = p * r + 1.0 / 6.0;
  p = p * r + 0.5;
  p = p * r + 1.0;
  p = p * r + 1.0;
  return ldexp(p, (int)kf);
}
