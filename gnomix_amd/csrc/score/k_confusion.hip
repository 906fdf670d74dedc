// score/k_confusion.hip — the confusion counts of a scored split, for labels and predictions that are already in HBM.
//
// Reference: Gnomix.train's bookkeeping (src/model.py:127-151) calls Base.evaluate / Smoother.evaluate (accuracy_score and
// balanced_accuracy_score of sklearn, src/Base/base.py:214-228, src/Smooth/smooth.py:67-79) and confusion_matrix
// (src/model.py:93-98) on label vectors.  All three are functions of the A x A table  cm[t, p] = #{i : y[i] == t, pred[i] == p},
// so a split that was predicted on the device needs only these A * A integers on the host (gnomix_amd/metrics.py finishes them).
//
// k_confusion<KIND>: a grid-stride pass, one element per thread and step.  The prediction is an int32 label, or the first-maximum
// argmax of a row of A probabilities (float64 / float32) as np.argmax(B, -1) of Base.evaluate takes it: a NaN counts as a maximum,
// the first NaN of a row wins.  Every workgroup counts into its own A x A table of 32-bit counters in LDS (one LDS add per element,
// no global traffic per element) and adds the table to the 64-bit global counters once, with one vector atomic per non-zero cell;
// it does so earlier whenever it has counted `flush_every` elements since the last time, so no 32-bit counter can pass 2^31.
// A true label or a predicted label outside [0, A) never indexes anything: it is counted in one extra cell.
#include "../gnx_internal.h"

namespace {

constexpr int CM_THREADS = 256;
constexpr int CM_MAX_A = GNX_CONFUSION_MAX_A;
constexpr int CM_PER_THREAD = 16;                       // elements a thread takes at least before the grid grows
constexpr int64_t CM_FLUSH_EVERY = (int64_t)1 << 31;    // elements a workgroup may count between two flushes

template <typename T>
__device__ __forceinline__ int32_t first_argmax(const T* __restrict__ row, int A) {
  // numpy's argmax loop: take v when !(v <= best), stop looking once best is a NaN
  T best = row[0];
  int32_t bi = 0;
  for (int a = 1; a < A && best == best; ++a) {
    const T v = row[a];
    if (!(v <= best)) {
      best = v;
      bi = a;
    }
  }
  return bi;
}

// extra[0] = elements with a label outside [0, A), extra[1] = flushes made (all workgroups)
template <int KIND>
__global__ __launch_bounds__(CM_THREADS) void k_confusion(const int32_t* __restrict__ y, const void* __restrict__ pred, int64_t n, int A,
                                                          uint32_t flush_every, unsigned long long* __restrict__ cm,
                                                          unsigned long long* __restrict__ extra) {
  __shared__ uint32_t tab[CM_MAX_A * CM_MAX_A + 1];
  const int cells = A * A;
  for (int c = threadIdx.x; c <= cells; c += CM_THREADS) tab[c] = 0;
  __syncthreads();
  auto flush = [&]() {  // the whole workgroup, between two barriers
    for (int c = threadIdx.x; c <= cells; c += CM_THREADS) {
      const uint32_t v = tab[c];
      if (v) atomicAdd(c < cells ? &cm[c] : &extra[0], (unsigned long long)v);
      tab[c] = 0;
    }
    if (threadIdx.x == 0) atomicAdd(&extra[1], 1ull);
  };
  uint32_t since = 0;  // elements this workgroup has counted since its last flush (an upper bound: the tail counts as full)
  const int64_t stride = (int64_t)gridDim.x * CM_THREADS;
  for (int64_t i0 = (int64_t)blockIdx.x * CM_THREADS; i0 < n; i0 += stride) {  // i0 is the same for the whole workgroup
    if (since + CM_THREADS > flush_every) {
      __syncthreads();
      flush();
      __syncthreads();
      since = 0;
    }
    const int64_t i = i0 + threadIdx.x;
    if (i < n) {
      const int32_t t = y[i];
      int32_t p;
      if (KIND == GNX_PRED_LABELS_I32) p = ((const int32_t*)pred)[i];
      else if (KIND == GNX_PRED_PROBA_F64) p = first_argmax((const double*)pred + i * A, A);
      else p = first_argmax((const float*)pred + i * A, A);
      const bool ok = t >= 0 && t < A && p >= 0 && p < A;
      atomicAdd(&tab[ok ? t * A + p : cells], 1u);
    }
    since += CM_THREADS;
  }
  __syncthreads();
  flush();
}

int confusion_check(gnx_ctx* ctx, const void* y, const void* pred, int pred_kind, int64_t n, int32_t A, const void* cm, int64_t flush_every) {
  if (!ctx->usable) return gnx_fail(ctx, GNX_ESTATE, "context has no device (gnx_init failed)");
  if (n < 0 || A < 1 || !cm || (n > 0 && (!y || !pred)))
    return gnx_fail(ctx, GNX_EINVAL, "confusion: need n >= 0, A >= 1, the counts' array and, for n > 0, y and pred");
  if (pred_kind != GNX_PRED_LABELS_I32 && pred_kind != GNX_PRED_PROBA_F64 && pred_kind != GNX_PRED_PROBA_F32)
    return gnx_fail(ctx, GNX_EINVAL, "confusion: pred_kind is GNX_PRED_LABELS_I32, GNX_PRED_PROBA_F64 or GNX_PRED_PROBA_F32");
  if (flush_every < 0) return gnx_fail(ctx, GNX_EINVAL, "confusion: debug_flush_every must be >= 0 (0 = the built-in 2^31)");
  if (A > CM_MAX_A)
    return gnx_fail(ctx, GNX_EUNSUPPORTED, "confusion: A = " + std::to_string(A) + " ancestries, the per-workgroup table holds " +
                                               std::to_string(CM_MAX_A) + " x " + std::to_string(CM_MAX_A) + " counters");
  return GNX_OK;
}

}  // namespace

extern "C" int gnx_confusion_dev(gnx_ctx* ctx, const int32_t* d_y, const void* d_pred, int pred_kind, int64_t n, int32_t A, int64_t* d_cm,
                                 int64_t debug_flush_every, int64_t* debug_n_flushes) {
  if (!ctx) return GNX_EINVAL;
  int rc = confusion_check(ctx, d_y, d_pred, pred_kind, n, A, d_cm, debug_flush_every);
  if (rc != GNX_OK) return rc;
  GNX_BIND_DEVICE(ctx);
  hipStream_t s = ctx->stream;
  HIPCHK(ctx, hipMemsetAsync(d_cm, 0, (size_t)A * A * sizeof(int64_t), s));
  if (debug_n_flushes) *debug_n_flushes = 0;
  if (n == 0) return GNX_OK;
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_misc, 2 * sizeof(unsigned long long))) != GNX_OK) return rc;
  unsigned long long* d_extra = (unsigned long long*)ctx->ws_misc.p;
  HIPCHK(ctx, hipMemsetAsync(d_extra, 0, 2 * sizeof(unsigned long long), s));
  // a workgroup counts at least CM_THREADS elements between two flushes, at most 2^31
  const int64_t fe = debug_flush_every ? std::min(std::max<int64_t>(debug_flush_every, CM_THREADS), CM_FLUSH_EVERY) : CM_FLUSH_EVERY;
  const int64_t per_block = (int64_t)CM_THREADS * CM_PER_THREAD;
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + per_block - 1) / per_block, (int64_t)ctx->n_cu * 8));
  unsigned long long* cm = (unsigned long long*)d_cm;
  if (pred_kind == GNX_PRED_LABELS_I32)
    hipLaunchKernelGGL(k_confusion<GNX_PRED_LABELS_I32>, dim3(grid), dim3(CM_THREADS), 0, s, d_y, d_pred, n, (int)A, (uint32_t)fe, cm, d_extra);
  else if (pred_kind == GNX_PRED_PROBA_F64)
    hipLaunchKernelGGL(k_confusion<GNX_PRED_PROBA_F64>, dim3(grid), dim3(CM_THREADS), 0, s, d_y, d_pred, n, (int)A, (uint32_t)fe, cm, d_extra);
  else
    hipLaunchKernelGGL(k_confusion<GNX_PRED_PROBA_F32>, dim3(grid), dim3(CM_THREADS), 0, s, d_y, d_pred, n, (int)A, (uint32_t)fe, cm, d_extra);
  HIPCHK(ctx, hipGetLastError());
  unsigned long long h_extra[2] = {0, 0};
  HIPCHK(ctx, hipMemcpyAsync(h_extra, d_extra, sizeof h_extra, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  if (debug_n_flushes) *debug_n_flushes = (int64_t)h_extra[1];
  if (h_extra[0])
    return gnx_fail(ctx, GNX_EINVAL, "confusion: " + std::to_string(h_extra[0]) + " of " + std::to_string(n) +
                                         " elements carry a label outside [0, " + std::to_string(A) + "); the counts hold the others");
  return GNX_OK;
}

extern "C" int gnx_confusion(gnx_ctx* ctx, const int32_t* y, const void* pred, int pred_kind, int64_t n, int32_t A, int64_t* cm,
                             int64_t debug_flush_every, int64_t* debug_n_flushes) {
  if (!ctx) return GNX_EINVAL;
  int rc = confusion_check(ctx, y, pred, pred_kind, n, A, cm, debug_flush_every);
  if (rc != GNX_OK) return rc;
  GNX_BIND_DEVICE(ctx);
  const size_t by = (size_t)n * sizeof(int32_t);
  const size_t bp = pred_kind == GNX_PRED_LABELS_I32 ? by : (size_t)n * A * (pred_kind == GNX_PRED_PROBA_F64 ? 8 : 4);
  const size_t bc = (size_t)A * A * sizeof(int64_t);
  gnx_devbuf& ws_pred = pred_kind == GNX_PRED_PROBA_F64 ? ctx->ws_p64 : ctx->ws_p32;
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_lab, by + 64)) != GNX_OK) return rc;
  if ((rc = gnx_ws_reserve(ctx, ws_pred, bp + 64)) != GNX_OK) return rc;
  // the counts live behind the kernel's own two cells in ws_misc (reserved here, so the device form's request does not move it)
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_misc, 256 + bc)) != GNX_OK) return rc;
  int64_t* d_cm = (int64_t*)((char*)ctx->ws_misc.p + 256);
  if (n > 0) {
    HIPCHK(ctx, hipMemcpyAsync(ctx->ws_lab.p, y, by, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ws_pred.p, pred, bp, hipMemcpyHostToDevice, ctx->stream));
  }
  rc = gnx_confusion_dev(ctx, (const int32_t*)ctx->ws_lab.p, ws_pred.p, pred_kind, n, A, d_cm, debug_flush_every,
                         debug_n_flushes);
  if (rc != GNX_OK && rc != GNX_EINVAL) return rc;
  // (GNX_EINVAL after the launch = labels out of range: the in-range counts are still handed over)
  const std::string msg = ctx->err;
  HIPCHK(ctx, hipMemcpyAsync(cm, d_cm, bc, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->err = msg;
  return rc;
}
