// gnx_window.h — the one home of window geometry: the base windows of Base.train_vectorized / predict_proba_vectorized (reference
// src/Base/base.py:41-44, 104-180) over the reflect-padded row, and the smoother's reflect padding over windows.  Every kernel file
// that walks either includes this header; none keeps a copy.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

// column of X behind position p of the row padded by reflection with ctx SNPs at both ends (p in [0, C + 2 ctx))
__host__ __device__ __forceinline__ int64_t gnx_pad_src(int64_t p, int64_t C, int64_t ctx) {
  if (p < ctx) return ctx - 1 - p;
  if (p < ctx + C) return p - ctx;
  return C - 1 - (p - ctx - C);
}

// window w covers padded positions [w M, w M + width): width = M + 2 ctx, the last window is rem = C - M W wider (it ends where the
// padded row ends)
__host__ __device__ __forceinline__ int64_t gnx_window_width(int64_t w, int64_t W, int64_t C, int64_t M, int64_t ctx) {
  return M + 2 * ctx + (w == W - 1 ? C - M * W : 0);
}

// window behind position j of the smoother's strip, padded by reflection with pad windows at both ends (j in [0, W + 2 pad)):
// slide_window (reference src/Smooth/utils.py:14-17)
__device__ __forceinline__ int gnx_slide_src(int j, int W, int pad) {
  if (j < pad) return pad - 1 - j;
  if (j < pad + W) return j - pad;
  return W - 1 - (j - pad - W);
}
