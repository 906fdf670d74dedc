// gnx_calibrate.h — "the calibrated probabilities / the calibrated label of one row": the ONE definition that k_calibrate.hip
// (Smoother.predict_proba with a calibrator) and k_gnofix_opts.hip (smoother.predict inside gnofix(), gnofix.py:80,190) share.
// Reference: src/Smooth/Calibration.py:57-69 -> sklearn IsotonicRegression(out_of_bounds="clip").transform per class, then
// Calibrator.normalize (:26-41), then np.argmax (src/Smooth/smooth.py:61).
//   per class c, as scikit-learn's transform does it: x is cast to the maps' type (a float64 input is NARROWED to float32 for maps
//   fitted in float32), clipped to [X_min, X_max], and interpolated on (X_thresholds_, y_thresholds_) as scipy's
//   interp1d(kind="linear") evaluates it, which depends on the maps' type:
//     float32 maps: interp1d's own form, every operation in float32: k = clip(searchsorted(x_thr, x, side="left"), 1, n-1),
//       slope = (y[k]-y[k-1])/(x[k]-x[k-1]),  y = slope*(x - x[k-1]) + y[k-1];
//     float64 maps (float32 inputs widened): np.interp: x == x_thr[k] returns y[k] itself, otherwise the same form on the bracket
//       x_thr[k-1] < x < x_thr[k] in float64.  (np.interp's NaN fallback needs a non-finite threshold: never with a fitted map.)
//   The value is then a float64;
//   normalize: 2 classes -> p0 = 1 - p1; else p /= np.sum(p) (in numpy's order of additions, see gnx_calib_row); NaN -> 1/A; (1, 1+1e-5] -> 1;  the first maximum wins.
// No per-thread array: a run-time-indexed double p[32] lives in scratch (272 B per lane).  A class's value is evaluated twice
// instead (once for the row sum, once for the output) — a few binary searches, and the same bits.
#pragma once
#include "gnx_internal.h"  // CalibMaps

// one class's interpolated value of the raw probability x (a float64 input, or a widened float32)
__device__ __forceinline__ double gnx_calib_value(const CalibMaps& M, int c, double x) {
  const int o0 = M.off[c], n = M.off[c + 1] - o0;
  const double* xs = M.x + o0;
  const double* ys = M.y + o0;
  if (n == 1) return ys[0];
  if (M.thr_f32) x = (double)(float)x;  // float32 maps: the input in float32 (thresholds are float32 values, so the clip and the search are too)
  x = fmin(fmax(x, xs[0]), xs[n - 1]);
  int lo = 0, hi = n;  // searchsorted(side="left"): first index with xs[idx] >= x
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (xs[mid] < x) lo = mid + 1; else hi = mid;
  }
  if (lo > n - 1) lo = n - 1;  // (never after the clip, unless a threshold is NaN)
  const int k = lo < 1 ? 1 : lo;
  if (M.thr_f32) {  // all operands are float32 values: same operations in float32
    const float xf = (float)x, x0 = (float)xs[k - 1], x1 = (float)xs[k], y0 = (float)ys[k - 1], y1 = (float)ys[k];
    const float slope = (y1 - y0) / (x1 - x0);
    return (double)(slope * (xf - x0) + y0);
  }
  if (xs[lo] == x) return ys[lo];  // np.interp: an exact hit is the threshold's own y
  const double slope = (ys[k] - ys[k - 1]) / (xs[k] - xs[k - 1]);
  return slope * (x - xs[k - 1]) + ys[k - 1];
}

// The calibrated row: raw(c) -> the row's raw probability of class c as a double (called up to twice per class, every class before
// the first emit), emit(c, p) receives the calibrated probability of class c in class order.  Returns the calibrated label.
template <class Raw, class Emit>
__device__ __forceinline__ int gnx_calib_row(const CalibMaps& M, int A, Raw raw, Emit emit) {
  // the row sum in np.sum's order over a contiguous row (numpy's pairwise sum, which for 8 <= A <= 128 is eight interleaved partial
  // sums combined as a tree, then the A % 8 last values one by one; below 8, one by one): with float64 values the order shows
  double sum = 0.0;
  if (A != 2 && A < 8) {
    for (int c = 0; c < A; ++c) sum += gnx_calib_value(M, c, raw(c));
  } else if (A != 2) {
    double r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = gnx_calib_value(M, j, raw(j));
    int c = 8;
    for (; c < A - (A & 7); c += 8) {
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] += gnx_calib_value(M, c + j, raw(c + j));
    }
    sum = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; c < A; ++c) sum += gnx_calib_value(M, c, raw(c));
  }
  const double p1 = (A == 2) ? gnx_calib_value(M, 1, raw(1)) : 0.0;
  int best = 0;
  double pbest = 0.0;
  for (int c = 0; c < A; ++c) {
    double pc = (A == 2) ? (c == 0 ? 1.0 - p1 : p1) : gnx_calib_value(M, c, raw(c)) / sum;
    if (pc != pc) pc = 1.0 / A;
    if (pc > 1.0 && pc <= 1.0 + 1e-5) pc = 1.0;
    if (c == 0 || pc > pbest) { best = c; pbest = pc; }   // first maximum wins, as np.argmax
    emit(c, pc);
  }
  return best;
}
