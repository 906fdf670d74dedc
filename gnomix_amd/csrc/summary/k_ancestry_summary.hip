// summary/k_ancestry_summary.hip — what users compute first from an .msp: global ancestry proportions per haplotype (the .Q table
// RFMix writes next to its .msp) and tract statistics per ancestry, for labels (and probabilities) that are in HBM.
//
// Per haplotype row n of W labels, window weights w (W float64, >= 0, e.g. the windows' lengths in cM) and ancestry a:
//   tract_total[n, a]   = sum of w[k] over the windows with lab[n, k] == a
//   hard[n, a]          = tract_total[n, a] / den,          den = sum of all w[k]  (computed once, on the host, in the same order)
//   soft[n, a]          = (sum of w[k] * P[n, k, a]) / den  (probabilities given; float32 values are widened before the multiply)
//   tract_count[n, a]   = number of maximal runs of label a in the row
//   tract_longest[n, a] = largest sum of w over one such run (0 when there is none)
//
// Work layout.  One wave per row, SM_ROWS rows per workgroup.  The wave stages its row once in LDS as bytes (labels are < 32; a
// label outside [0, A) is staged as 0xff, equals no class, and raises the flag the launcher reads back: labels are only compared,
// never used as an index).  With L = ceil(W / 64), lane c owns the contiguous chunk of windows [c L, min(W, (c + 1) L)) (the last
// lanes own nothing when W < 64 L).  Nothing per class lives in a per-thread array (a runtime-indexed one is scratch memory):
// the wave goes through the classes one after another and recomputes from the staged row; lane 0 writes the class's five results.
//
// SUMMATION ORDER (tests/summary_exact.py restates exactly this).  It depends on W alone, never on the launch geometry.
//   * A sum over windows (tract_total, the soft numerator, den): every lane adds its chunk's terms left to right onto 0.0 (a
//     window that does not belong to the class is skipped; a soft term is the rounded product w[k] * P, no fused multiply-add); the 64
//     lane values t[0..63] are then folded in six steps, d = 32, 16, 8, 4, 2, 1: t[c] = t[c] + t[c + d] for c < d; t[0] is the sum.
//   * The length of a run.  Inside a chunk a run's windows are added left to right, the first term as it is.  A run that goes on
//     past its chunk's end leaves its piece in the lane's value v[c] (0.0 otherwise), with the flag f[c] = 0 when that piece began at
//     the chunk's first window as the continuation of a run of the lane before (the lane's whole chunk is then the inside of one
//     run), else f[c] = 1.  An inclusive segmented scan (Hillis-Steele) over the lanes follows, d = 1, 2, 4, 8, 16, 32, all lanes
//     at once from the values before the step:  if c >= d and f[c] == 0: v[c] = v[c - d] + v[c];  if c >= d: f[c] |= f[c - d].
//     carry[c] = v[c - 1] after the scan (0.0 for lane 0).  A run that began in its lane has the length of its piece; a run that
//     came in from the lane before has the length carry[c] + piece.  A run is counted, and its length compared with the longest,
//     by the lane that holds its last window.
//   * hard, soft: one division by den.  The longest run is a maximum: no rounding, any order.
//
// No scratch, no atomics on floating-point values (the one atomic is the integer error flag); every output word is written by
// exactly one lane, so two calls on the same input give the same bits.
#include "../gnx_internal.h"

namespace {

constexpr int SM_THREADS = 256;
constexpr int SM_ROWS = SM_THREADS / 64;       // one wave per row
constexpr int SM_MAX_W = GNX_SUMMARY_MAX_W;    // labels a wave stages (1 byte each): SM_ROWS * SM_MAX_W bytes of LDS
constexpr int SM_MAX_A = GNX_SUMMARY_MAX_A;

// t[0] of the fold above, in every lane
__device__ __forceinline__ double fold_sum(double v) {
  for (int d = 32; d > 0; d >>= 1) v = __dadd_rn(v, __shfl_down(v, d, 64));
  return __shfl(v, 0, 64);
}
__device__ __forceinline__ double fold_max(double v) {
  for (int d = 32; d > 0; d >>= 1) v = fmax(v, __shfl_down(v, d, 64));
  return __shfl(v, 0, 64);
}
__device__ __forceinline__ int fold_add(int v) {
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  return __shfl(v, 0, 64);
}

// lab (N, ldl) int32; P (N, W, A) float32 / float64 or NULL; w (W) float64; outputs (N, A), each may be NULL
template <typename TP>
__global__ __launch_bounds__(SM_THREADS) void k_ancestry_summary(const int32_t* __restrict__ lab, int64_t ldl, const TP* __restrict__ P,
                                                                 const double* __restrict__ w, double den, int64_t N, int W, int A,
                                                                 double* __restrict__ hard, double* __restrict__ soft,
                                                                 int32_t* __restrict__ t_count, double* __restrict__ t_total,
                                                                 double* __restrict__ t_longest, unsigned int* __restrict__ bad) {
  __shared__ uint8_t tile[SM_ROWS * SM_MAX_W];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * SM_ROWS + wv;
  uint8_t* row = tile + wv * SM_MAX_W;
  if (r < N) {
    const int32_t* g = lab + r * ldl;
    bool any_bad = false;
    for (int k = lane; k < W; k += 64) {
      const int32_t v = g[k];
      const bool ok = v >= 0 && v < A;
      any_bad |= !ok;
      row[k] = ok ? (uint8_t)v : (uint8_t)0xff;
    }
    if (any_bad) atomicOr(bad, 1u);  // (at most one per thread, and only for malformed input)
  }
  __syncthreads();
  if (r >= N) return;  // (whole waves leave: no barrier follows)

  const int L = (W + 63) >> 6;
  const int k0 = min(W, lane * L), k1 = min(W, k0 + L);  // this lane's chunk (empty for the last lanes when W < 64 L)
  const TP* prow = P ? P + (size_t)r * (size_t)W * (size_t)A : nullptr;
  for (int a = 0; a < A; ++a) {
    double tot = 0.0, lng = 0.0, run = 0.0, head = 0.0;
    int cnt = 0;
    bool open = false, from_prev = false, head_closed = false;
    const bool prev_is = k0 > 0 && k0 < W && row[k0 - 1] == a;
    for (int k = k0; k < k1; ++k) {
      if (row[k] == a) {
        const double wk = w[k];
        tot = __dadd_rn(tot, wk);
        if (!open) {
          open = true;
          run = wk;
          from_prev = k == k0 && prev_is;
        } else {
          run = __dadd_rn(run, wk);
        }
      } else {
        if (open) {  // the run ended at k - 1, inside this chunk
          if (from_prev) {
            head = run;  // its length needs the carry: after the scan
            head_closed = true;
          } else {
            ++cnt;
            lng = fmax(lng, run);
          }
          open = false;
        }
      }
    }
    // the piece that is open at the chunk's end: does its run go on in the next lane?
    const bool goes_on = open && k1 < W && row[k1] == a;
    double v = goes_on ? run : 0.0;
    int f = (goes_on && from_prev) ? 0 : 1;
    for (int d = 1; d < 64; d <<= 1) {
      const double vu = __shfl_up(v, d, 64);
      const int fu = __shfl_up(f, d, 64);
      if (lane >= d) {
        if (!f) v = __dadd_rn(vu, v);
        f |= fu;
      }
    }
    double carry = __shfl_up(v, 1, 64);
    if (lane == 0) carry = 0.0;
    if (head_closed) {
      ++cnt;
      lng = fmax(lng, __dadd_rn(carry, head));
    }
    if (open && !goes_on) {  // its last window is this chunk's last
      ++cnt;
      lng = fmax(lng, from_prev ? __dadd_rn(carry, run) : run);
    }
    tot = fold_sum(tot);
    if (t_longest) lng = fold_max(lng);
    if (t_count) cnt = fold_add(cnt);
    double sp = 0.0;
    if (prow) {
      for (int k = k0; k < k1; ++k) sp = __dadd_rn(sp, __dmul_rn(w[k], (double)prow[(size_t)k * A + a]));
      sp = fold_sum(sp);
    }
    if (lane == 0) {
      const int64_t o = r * A + a;
      if (hard) hard[o] = __ddiv_rn(tot, den);
      if (prow) soft[o] = __ddiv_rn(sp, den);
      if (t_count) t_count[o] = cnt;
      if (t_total) t_total[o] = tot;
      if (t_longest) t_longest[o] = lng;
    }
  }
}

// den in the order of the kernel's sums over windows (the file header), on the host
double host_den(const double* w, int64_t W) {
  const int64_t L = (W + 63) / 64;
  volatile double t[64];  // (volatile: every addition is rounded to float64 and none is reassociated)
  for (int c = 0; c < 64; ++c) {
    double s = 0.0;
    for (int64_t k = std::min(W, c * L); k < std::min(W, (c + 1) * L); ++k) s = s + w[k];
    t[c] = s;
  }
  for (int d = 32; d > 0; d >>= 1)
    for (int c = 0; c < d; ++c) t[c] = t[c] + t[c + d];
  return t[0];
}

// the argument checks of both forms; on GNX_OK *wts holds the weights (all ones for weights == NULL) and *den their sum
int summary_check(gnx_ctx* ctx, const void* labels, int64_t ldl, const void* proba, const double* weights, int64_t N, int64_t W, int32_t A,
                  const void* soft, std::vector<double>* wts, double* den) {
  if (!ctx->usable) return gnx_fail(ctx, GNX_ESTATE, "context has no device (gnx_init failed)");
  if (N < 0 || W < 1 || A < 1) return gnx_fail(ctx, GNX_EINVAL, "ancestry_summary: need N >= 0, W >= 1 and A >= 1");
  if (ldl < W) return gnx_fail(ctx, GNX_EINVAL, "ancestry_summary: the labels' row stride is smaller than W");
  if ((proba == nullptr) != (soft == nullptr))
    return gnx_fail(ctx, GNX_EINVAL, "ancestry_summary: the soft proportions and the probabilities are given together or not at all");
  if (N > 0 && !labels) return gnx_fail(ctx, GNX_EINVAL, "ancestry_summary: no labels");
  if (A > SM_MAX_A)
    return gnx_fail(ctx, GNX_EUNSUPPORTED, "ancestry_summary: A = " + std::to_string(A) + " ancestries, a staged label is compared with at most " +
                                               std::to_string(SM_MAX_A) + " classes");
  if (W > SM_MAX_W)
    return gnx_fail(ctx, GNX_EUNSUPPORTED, "ancestry_summary: W = " + std::to_string(W) + " windows, a wave stages a row of at most " +
                                               std::to_string(SM_MAX_W) + " labels in LDS");
  if (N > ((int64_t)1 << 31) * SM_ROWS - SM_ROWS) return gnx_fail(ctx, GNX_EUNSUPPORTED, "ancestry_summary: more rows than one grid takes");
  wts->assign((size_t)W, 1.0);
  if (weights) {
    for (int64_t k = 0; k < W; ++k) {
      const double v = weights[k];
      if (!(v >= 0.0) || !(v <= 1.7976931348623157e308))
        return gnx_fail(ctx, GNX_EINVAL, "ancestry_summary: weight " + std::to_string(k) + " is negative or not finite");
      (*wts)[(size_t)k] = v;
    }
  }
  *den = host_den(wts->data(), W);
  if (!(*den > 0.0)) return gnx_fail(ctx, GNX_EINVAL, "ancestry_summary: the weights sum to zero");
  if (!(*den <= 1.7976931348623157e308)) return gnx_fail(ctx, GNX_EINVAL, "ancestry_summary: the weights' sum is not finite");
  return GNX_OK;
}

// the launch and the verdict on the labels; wts / den from summary_check
int summary_run(gnx_ctx* ctx, const int32_t* d_labels, int64_t ldl, const void* d_proba, int proba_is_f64, const std::vector<double>& wts,
                double den, int64_t N, int64_t W, int32_t A, double* d_hard, double* d_soft, int32_t* d_count, double* d_total,
                double* d_longest) {
  int rc;
  hipStream_t s = ctx->stream;
  // ws_misc: the error flag, then (256 bytes on) the weights
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_misc, 256 + (size_t)W * sizeof(double))) != GNX_OK) return rc;
  unsigned int* d_bad = (unsigned int*)ctx->ws_misc.p;
  double* d_w = (double*)((char*)ctx->ws_misc.p + 256);
  HIPCHK(ctx, hipMemsetAsync(d_bad, 0, sizeof(unsigned int), s));
  HIPCHK(ctx, hipMemcpyAsync(d_w, wts.data(), (size_t)W * sizeof(double), hipMemcpyHostToDevice, s));
  const unsigned grid = (unsigned)((N + SM_ROWS - 1) / SM_ROWS);
  if (d_proba && !proba_is_f64)
    hipLaunchKernelGGL(k_ancestry_summary<float>, dim3(grid), dim3(SM_THREADS), 0, s, d_labels, ldl, (const float*)d_proba, (const double*)d_w,
                       den, N, (int)W, (int)A, d_hard, d_soft, d_count, d_total, d_longest, d_bad);
  else
    hipLaunchKernelGGL(k_ancestry_summary<double>, dim3(grid), dim3(SM_THREADS), 0, s, d_labels, ldl, (const double*)d_proba, (const double*)d_w,
                       den, N, (int)W, (int)A, d_hard, d_soft, d_count, d_total, d_longest, d_bad);
  HIPCHK(ctx, hipGetLastError());
  unsigned int h_bad = 0;
  HIPCHK(ctx, hipMemcpyAsync(&h_bad, d_bad, sizeof h_bad, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));  // (the host copy of the weights is no longer needed after this either)
  if (h_bad)
    return gnx_fail(ctx, GNX_EINVAL, "ancestry_summary: a label lies outside [0, " + std::to_string(A) + "); such a label counts for no ancestry");
  return GNX_OK;
}

}  // namespace

extern "C" int gnx_ancestry_summary_dev(gnx_ctx* ctx, const int32_t* d_labels, int64_t ld_labels, const void* d_proba, int proba_is_f64,
                                        const double* weights, int64_t N, int64_t W, int32_t A, double* d_hard, double* d_soft,
                                        int32_t* d_tract_count, double* d_tract_total, double* d_tract_longest) {
  if (!ctx) return GNX_EINVAL;
  std::vector<double> wts;
  double den = 0.0;
  int rc = summary_check(ctx, d_labels, ld_labels, d_proba, weights, N, W, A, d_soft, &wts, &den);
  if (rc != GNX_OK) return rc;
  if (N == 0) return GNX_OK;
  GNX_BIND_DEVICE(ctx);
  return summary_run(ctx, d_labels, ld_labels, d_proba, proba_is_f64, wts, den, N, W, A, d_hard, d_soft, d_tract_count, d_tract_total,
                     d_tract_longest);
}

extern "C" int gnx_ancestry_summary(gnx_ctx* ctx, const int32_t* labels, int64_t ld_labels, const void* proba, int proba_is_f64,
                                    const double* weights, int64_t N, int64_t W, int32_t A, double* hard, double* soft, int32_t* tract_count,
                                    double* tract_total, double* tract_longest) {
  if (!ctx) return GNX_EINVAL;
  std::vector<double> wts;
  double den = 0.0;
  int rc = summary_check(ctx, labels, ld_labels, proba, weights, N, W, A, soft, &wts, &den);
  if (rc != GNX_OK) return rc;
  if (N == 0) return GNX_OK;
  GNX_BIND_DEVICE(ctx);
  hipStream_t s = ctx->stream;
  const size_t bl = ((size_t)(N - 1) * (size_t)ld_labels + (size_t)W) * sizeof(int32_t);  // the last row ends after its W labels
  const size_t bp = proba ? (size_t)N * (size_t)W * (size_t)A * (proba_is_f64 ? 8 : 4) : 0;
  const size_t na = (size_t)N * (size_t)A, bd = (na * sizeof(double) + 255) & ~(size_t)255, bi = (na * sizeof(int32_t) + 255) & ~(size_t)255;
  gnx_devbuf& ws_proba = proba_is_f64 ? ctx->ws_p64 : ctx->ws_p32;
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_lab, bl + 64)) != GNX_OK) return rc;
  if (proba && (rc = gnx_ws_reserve(ctx, ws_proba, bp + 64)) != GNX_OK) return rc;
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_b64, 4 * bd + bi)) != GNX_OK) return rc;
  char* o = (char*)ctx->ws_b64.p;
  double* d_hard = hard ? (double*)o : nullptr;
  double* d_soft = soft ? (double*)(o + bd) : nullptr;
  double* d_total = tract_total ? (double*)(o + 2 * bd) : nullptr;
  double* d_longest = tract_longest ? (double*)(o + 3 * bd) : nullptr;
  int32_t* d_count = tract_count ? (int32_t*)(o + 4 * bd) : nullptr;
  HIPCHK(ctx, hipMemcpyAsync(ctx->ws_lab.p, labels, bl, hipMemcpyHostToDevice, s));
  if (proba) HIPCHK(ctx, hipMemcpyAsync(ws_proba.p, proba, bp, hipMemcpyHostToDevice, s));
  rc = summary_run(ctx, (const int32_t*)ctx->ws_lab.p, ld_labels, proba ? ws_proba.p : nullptr, proba_is_f64, wts, den, N, W, A, d_hard, d_soft,
                   d_count, d_total, d_longest);
  if (rc != GNX_OK && rc != GNX_EINVAL) return rc;
  // (GNX_EINVAL after the launch = labels out of range: the results of the other labels are still handed over)
  const std::string msg = ctx->err;
  if (hard) HIPCHK(ctx, hipMemcpyAsync(hard, d_hard, na * sizeof(double), hipMemcpyDeviceToHost, s));
  if (soft) HIPCHK(ctx, hipMemcpyAsync(soft, d_soft, na * sizeof(double), hipMemcpyDeviceToHost, s));
  if (tract_total) HIPCHK(ctx, hipMemcpyAsync(tract_total, d_total, na * sizeof(double), hipMemcpyDeviceToHost, s));
  if (tract_longest) HIPCHK(ctx, hipMemcpyAsync(tract_longest, d_longest, na * sizeof(double), hipMemcpyDeviceToHost, s));
  if (tract_count) HIPCHK(ctx, hipMemcpyAsync(tract_count, d_count, na * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  ctx->err = msg;
  return rc;
}
