// gnx_window.h — the window geometry of Base.train_vectorized / predict_proba_vectorized (reference src/Base/base.py:41-44, 104-180), one
// definition for the kernels that walk a window's slice of the reflect-padded row (nb/k_base_nb.hip, lda/k_train_lda.hip, lda/k_base_lda.hip).
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
