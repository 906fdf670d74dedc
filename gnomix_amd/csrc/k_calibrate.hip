// k_calibrate.hip — Calibrator.transform on gfx950 (reference src/Smooth/Calibration.py:57-69 -> sklearn
// IsotonicRegression(out_of_bounds="clip").transform per class, then Calibrator.normalize, :26-41).
// The row arithmetic (clip, interpolate in the fitted type, normalise, NaN, clamp, first maximum) is gnx_calibrate.h, shared with
// the Gnofix kernel that labels a calibrated model's rows (k_gnofix_opts.hip).  One thread per row.
#include "gnx_internal.h"
#include "gnx_calibrate.h"

namespace {

__global__ __launch_bounds__(256) void k_calibrate(CalibLaunch L) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= L.R) return;
  const int A = L.A;
  const CalibMaps M{L.off, L.x, L.y, L.thr_f32};
  // (out64 may alias `in`: gnx_calib_row has read every input of the row for the sum before the first emit, and re-reads class
  //  c's own value before emit(c) overwrites it)
  const int best = gnx_calib_row(
      M, A,
      [&](int c) -> double {
        return L.in_is_f64 ? reinterpret_cast<const double*>(L.in)[r * A + c] : (double)reinterpret_cast<const float*>(L.in)[r * A + c];
      },
      [&](int c, double pc) {
        if (L.out64) L.out64[r * A + c] = pc;
        if (L.out32) L.out32[r * A + c] = (float)pc;
      });
  if (L.labels) L.labels[r] = best;
}

}  // namespace

hipError_t gnx_launch_calibrate(const CalibLaunch& L, hipStream_t s) {
  if (L.R <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_calibrate, dim3((unsigned)((L.R + 255) / 256)), dim3(256), 0, s, L);
  return hipGetLastError();
}
