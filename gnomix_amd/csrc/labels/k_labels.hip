// labels/k_labels.hip — what the reference does with the window labels after the smoother's argmax, for labels that are in HBM.
//
// Reference: Smoother.predict's mode_filter (src/Smooth/smooth.py:58-65, src/Smooth/utils.py:31-46) and the run-length encoding
// of a haplotype's labels that get_bed_data computes for the .bed files (src/postprocess.py:162-193).
//
// k_mode_filter.  Per row `pred` of W labels and ends = size / 2, position i with ends <= i < W - ends (and ends > 0) becomes the mode
// of pred[i - ends .. i + ends] when that mode is unambiguous, and stays pred[i] otherwise; every other position is copied.  The
// window is always read from the INPUT row (the reference filters out of `pred` into a copy: nothing cascades).  "Unambiguous" is the
// reference's test under the scipy it was written for: the smallest most frequent label (stats.mode(arr)[0][0]) equals the largest
// most frequent one (-stats.mode(-arr)[0][0]).  A workgroup takes `rpb` whole rows, stages them once in LDS as bytes (labels are
// < GNX_MODE_FILTER_MAX_A = 32) and runs one thread per output position: for each class in ascending order the thread counts the class
// in its window; a strict > on the count keeps the smallest best class, >= the largest.  The counts are recomputed per class
// instead of being held in A per-thread counters (a runtime-indexed per-thread array is scratch memory: k_calibrate's lesson).
// A row longer than the LDS tile (MF_LDS_BYTES labels) is not staged: the same kernel then reads its windows from global memory
// (they stay in L1 / L2: neighbouring threads read neighbouring windows).  A label outside [0, A) indexes nothing (labels are only
// ever compared); it raises the error flag the launcher reads back.
//
// k_label_runs_count / k_label_runs_scan / k_label_runs_fill.  A run is a maximal stretch of equal labels in a row.  One wave per
// row counts the run starts (w == 0 or pred[w] != pred[w - 1]); one workgroup turns the N counts into their exclusive prefix; one
// wave per row then writes the (first_window, last_window, label) triples at prefix[row] + rank, where rank is the run's number in
// its row, taken from a ballot of the wave's run starts.  The lane that starts run k also closes run k - 1 (last = w - 1), so every
// word is written by exactly one lane: no atomics.
#include "../gnx_internal.h"

namespace {

constexpr int MF_THREADS = 256;
constexpr int MF_LDS_BYTES = GNX_MODE_FILTER_LDS_ROW;  // labels a workgroup stages (1 byte each); a longer row takes the global path
constexpr int MF_MAX_A = GNX_MODE_FILTER_MAX_A;
constexpr int LR_THREADS = 256;
constexpr int LR_ROWS = LR_THREADS / 64;  // one wave per row

// the filter's verdict on one window [p - ends, p + ends] of a row; get(j) = label at position j
template <class Get>
__device__ __forceinline__ int32_t window_mode(Get&& get, int64_t p, int ends, int A, int32_t centre) {
  int best = -1, lo = 0, hi = 0;
  for (int a = 0; a < A; ++a) {
    int cnt = 0;
    for (int64_t j = p - ends; j <= p + ends; ++j) cnt += get(j) == a ? 1 : 0;
    if (cnt > best) {
      best = cnt;
      lo = a;
    }
    if (cnt >= best) hi = a;  // (best was just raised when cnt > best)
  }
  return lo == hi ? lo : centre;
}

// in (N, ldi) int32 -> out (N, ldo) int32.  staged: rows of W <= MF_LDS_BYTES labels, rpb rows per workgroup through LDS;
// otherwise a grid-stride pass over the N * W positions that reads global memory.  ends > 0 and 2 * ends < W, or ends == 0: copy.
__global__ __launch_bounds__(MF_THREADS) void k_mode_filter(const int32_t* __restrict__ in, int64_t ldi, int32_t* __restrict__ out, int64_t ldo,
                                                            int64_t N, int W, int ends, int A, int rpb, int staged,
                                                            unsigned int* __restrict__ bad) {
  __shared__ uint8_t tile[MF_LDS_BYTES];
  bool any_bad = false;
  if (staged) {
    const int64_t r0 = (int64_t)blockIdx.x * rpb;
    const int rows = (int)(N - r0 < rpb ? N - r0 : rpb);  // rows * W <= MF_LDS_BYTES
    const int n = rows * W;
    for (int k = threadIdx.x; k < n; k += MF_THREADS) {
      const int r = k / W, i = k - r * W;
      const int32_t v = in[(r0 + r) * ldi + i];
      const bool ok = v >= 0 && v < A;
      any_bad |= !ok;
      tile[k] = ok ? (uint8_t)v : (uint8_t)0xff;  // 0xff equals no class
    }
    __syncthreads();
    for (int k = threadIdx.x; k < n; k += MF_THREADS) {
      const int r = k / W, i = k - r * W;
      const uint8_t* row = tile + r * W;
      int32_t v = row[i];
      if (v == 0xff) v = in[(r0 + r) * ldi + i];  // an out-of-range label is handed on as it came
      else if (ends > 0 && i >= ends && i < W - ends)
        v = window_mode([&](int64_t j) { return (int)row[j]; }, i, ends, A, v);
      out[(r0 + r) * ldo + i] = v;
    }
  } else {
    const int64_t total = N * (int64_t)W, stride = (int64_t)gridDim.x * MF_THREADS;
    for (int64_t k = (int64_t)blockIdx.x * MF_THREADS + threadIdx.x; k < total; k += stride) {
      const int64_t r = k / W, i = k - r * W;
      const int32_t* row = in + r * ldi;
      int32_t v = row[i];
      const bool ok = v >= 0 && v < A;
      any_bad |= !ok;
      if (ok && ends > 0 && i >= ends && i < W - ends) v = window_mode([&](int64_t j) { return row[j]; }, i, ends, A, v);
      out[r * ldo + i] = v;
    }
  }
  if (any_bad) atomicOr(bad, 1u);  // (at most one per thread, and only for malformed input)
}

__device__ __forceinline__ int wave_sum(int v) {
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  return __shfl(v, 0, 64);
}

__global__ __launch_bounds__(LR_THREADS) void k_label_runs_count(const int32_t* __restrict__ lab, int64_t ldl, int64_t N, int W,
                                                                 int64_t* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * LR_ROWS + (threadIdx.x >> 6);
  if (r >= N) return;  // (whole waves leave: no barrier follows)
  const int32_t* row = lab + r * ldl;
  int c = 0;
  for (int w = lane; w < W; w += 64) c += (w == 0 || row[w] != row[w - 1]) ? 1 : 0;
  c = wave_sum(c);
  if (lane == 0) counts[r] = c;
}

// off[0 .. N] = exclusive prefix of counts[0 .. N) and, in off[N], the total; one workgroup, each thread a contiguous share
__global__ __launch_bounds__(LR_THREADS) void k_label_runs_scan(const int64_t* __restrict__ counts, int64_t N, int64_t* __restrict__ off) {
  __shared__ int64_t part[LR_THREADS];
  const int64_t per = (N + LR_THREADS - 1) / LR_THREADS;
  const int64_t a = std::min<int64_t>(N, (int64_t)threadIdx.x * per), b = std::min<int64_t>(N, a + per);
  int64_t s = 0;
  for (int64_t i = a; i < b; ++i) s += counts[i];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t run = 0;
    for (int t = 0; t < LR_THREADS; ++t) {
      const int64_t v = part[t];
      part[t] = run;
      run += v;
    }
    off[N] = run;
  }
  __syncthreads();
  s = part[threadIdx.x];
  for (int64_t i = a; i < b; ++i) {
    off[i] = s;
    s += counts[i];
  }
}

__global__ __launch_bounds__(LR_THREADS) void k_label_runs_fill(const int32_t* __restrict__ lab, int64_t ldl, int64_t N, int W,
                                                                const int64_t* __restrict__ off, int32_t* __restrict__ triples) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * LR_ROWS + (threadIdx.x >> 6);
  if (r >= N || W <= 0) return;
  const int32_t* row = lab + r * ldl;
  int32_t* t = triples + 3 * off[r];
  int base = 0;  // runs of this row that started before the current step
  for (int w0 = 0; w0 < W; w0 += 64) {  // w0 is the same for the whole wave
    const int w = w0 + lane;
    const bool start = w < W && (w == 0 || row[w] != row[w - 1]);
    const unsigned long long m = __ballot(start);
    if (start) {
      const int k = base + __popcll(m & ((1ull << lane) - 1ull));
      t[3 * k] = w;
      t[3 * k + 2] = row[w];
      if (k > 0) t[3 * (k - 1) + 1] = w - 1;  // closes the run before (k > 0 <=> w > 0)
    }
    base += __popcll(m);
  }
  if (lane == 0) t[3 * (base - 1) + 1] = W - 1;
}

int mode_filter_check(gnx_ctx* ctx, const void* in, const void* out, int64_t N, int64_t W, int32_t A, int64_t size) {
  if (!ctx->usable) return gnx_fail(ctx, GNX_ESTATE, "context has no device (gnx_init failed)");
  if (N < 0 || W < 0 || W > INT32_MAX || A < 1 || size < 0 || (N > 0 && W > 0 && (!in || !out)))
    return gnx_fail(ctx, GNX_EINVAL, "mode_filter: need N >= 0, 0 <= W < 2^31, A >= 1, size >= 0 and, for N * W > 0, both label arrays");
  if (A > MF_MAX_A)
    return gnx_fail(ctx, GNX_EUNSUPPORTED, "mode_filter: A = " + std::to_string(A) + " ancestries, a staged label is compared with at most " +
                                               std::to_string(MF_MAX_A) + " classes");
  return GNX_OK;
}

// counts (N) and off (N + 1) on the device; *total on the host (one synchronisation)
int runs_count(gnx_ctx* ctx, const int32_t* d_lab, int64_t ldl, int64_t N, int64_t W, int64_t* d_counts, int64_t* d_off, int64_t* total) {
  hipStream_t s = ctx->stream;
  const unsigned grid = (unsigned)((N + LR_ROWS - 1) / LR_ROWS);
  hipLaunchKernelGGL(k_label_runs_count, dim3(grid), dim3(LR_THREADS), 0, s, d_lab, ldl, N, (int)W, d_counts);
  HIPCHK(ctx, hipGetLastError());
  hipLaunchKernelGGL(k_label_runs_scan, dim3(1), dim3(LR_THREADS), 0, s, (const int64_t*)d_counts, N, d_off);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(total, d_off + N, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  return GNX_OK;
}

int runs_fill(gnx_ctx* ctx, const int32_t* d_lab, int64_t ldl, int64_t N, int64_t W, const int64_t* d_off, int32_t* d_triples) {
  const unsigned grid = (unsigned)((N + LR_ROWS - 1) / LR_ROWS);
  hipLaunchKernelGGL(k_label_runs_fill, dim3(grid), dim3(LR_THREADS), 0, ctx->stream, d_lab, ldl, N, (int)W, d_off, d_triples);
  HIPCHK(ctx, hipGetLastError());
  return GNX_OK;
}

int label_runs_check(gnx_ctx* ctx, const void* lab, int64_t ldl, int64_t N, int64_t W, const void* counts, const void* off,
                     const void* triples, int64_t cap, const void* total) {
  if (!ctx->usable) return gnx_fail(ctx, GNX_ESTATE, "context has no device (gnx_init failed)");
  if (N < 0 || W < 0 || W > INT32_MAX || ldl < W || cap < 0 || !counts || !off || !total || (cap > 0 && !triples) || (N > 0 && W > 0 && !lab) ||
      N > ((int64_t)1 << 31) * LR_ROWS - LR_ROWS)
    return gnx_fail(ctx, GNX_EINVAL, "label_runs: need N >= 0, 0 <= W < 2^31, ld >= W, capacity >= 0, the labels and every output array");
  return GNX_OK;
}

int too_small(gnx_ctx* ctx, int64_t total, int64_t cap) {
  return gnx_fail(ctx, GNX_EINVAL, "label_runs: the labels hold " + std::to_string(total) + " runs, the triples' array has room for " +
                                       std::to_string(cap) + "; the counts and their prefix are written, the triples are not");
}

}  // namespace

extern "C" int gnx_mode_filter_dev(gnx_ctx* ctx, const int32_t* d_in, int64_t ld_in, int32_t* d_out, int64_t ld_out, int64_t N, int64_t W,
                                   int32_t A, int64_t size) {
  if (!ctx) return GNX_EINVAL;
  int rc = mode_filter_check(ctx, d_in, d_out, N, W, A, size);
  if (rc != GNX_OK) return rc;
  if (ld_in < W || ld_out < W) return gnx_fail(ctx, GNX_EINVAL, "mode_filter: a row stride is smaller than W");
  if (N == 0 || W == 0) return GNX_OK;
  GNX_BIND_DEVICE(ctx);
  hipStream_t s = ctx->stream;
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_misc, sizeof(unsigned int))) != GNX_OK) return rc;
  unsigned int* d_bad = (unsigned int*)ctx->ws_misc.p;
  HIPCHK(ctx, hipMemsetAsync(d_bad, 0, sizeof(unsigned int), s));
  int64_t ends = size / 2;
  if (2 * ends >= W) ends = 0;  // range(W)[ends:-ends] is empty: every label is kept (and the window offsets stay small)
  const int staged = W <= MF_LDS_BYTES;
  int rpb = 1;
  unsigned grid;
  if (staged) {
    // whole rows per workgroup: as many as the tile holds, fewer while that leaves CUs without a workgroup
    const int64_t fit = MF_LDS_BYTES / W, spread = (N + (int64_t)ctx->n_cu * 4 - 1) / ((int64_t)ctx->n_cu * 4);
    rpb = (int)std::max<int64_t>(1, std::min(fit, spread));
    if (N > (int64_t)rpb * INT32_MAX) return gnx_fail(ctx, GNX_EUNSUPPORTED, "mode_filter: more rows than one grid takes");
    grid = (unsigned)((N + rpb - 1) / rpb);
  } else {
    const int64_t per_block = (int64_t)MF_THREADS * 4;
    grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((N * W + per_block - 1) / per_block, (int64_t)ctx->n_cu * 16));
  }
  hipLaunchKernelGGL(k_mode_filter, dim3(grid), dim3(MF_THREADS), 0, s, d_in, ld_in, d_out, ld_out, N, (int)W, (int)ends, (int)A, rpb, staged,
                     d_bad);
  HIPCHK(ctx, hipGetLastError());
  unsigned int h_bad = 0;
  HIPCHK(ctx, hipMemcpyAsync(&h_bad, d_bad, sizeof h_bad, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  if (h_bad)
    return gnx_fail(ctx, GNX_EINVAL, "mode_filter: a label lies outside [0, " + std::to_string(A) + "); such labels are handed on unchanged");
  return GNX_OK;
}

extern "C" int gnx_mode_filter(gnx_ctx* ctx, const int32_t* in, int32_t* out, int64_t N, int64_t W, int32_t A, int64_t size) {
  if (!ctx) return GNX_EINVAL;
  int rc = mode_filter_check(ctx, in, out, N, W, A, size);
  if (rc != GNX_OK) return rc;
  if (N == 0 || W == 0) return GNX_OK;
  GNX_BIND_DEVICE(ctx);
  const size_t by = (size_t)N * (size_t)W * sizeof(int32_t), half = (by + 255) & ~(size_t)255;
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_lab, 2 * half)) != GNX_OK) return rc;
  int32_t* d_in = (int32_t*)ctx->ws_lab.p;
  int32_t* d_out = (int32_t*)((char*)ctx->ws_lab.p + half);
  HIPCHK(ctx, hipMemcpyAsync(d_in, in, by, hipMemcpyHostToDevice, ctx->stream));
  rc = gnx_mode_filter_dev(ctx, d_in, W, d_out, W, N, W, A, size);
  if (rc != GNX_OK && rc != GNX_EINVAL) return rc;
  const std::string msg = ctx->err;
  HIPCHK(ctx, hipMemcpyAsync(out, d_out, by, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->err = msg;
  return rc;
}

extern "C" int gnx_label_runs_dev(gnx_ctx* ctx, const int32_t* d_labels, int64_t ldl, int64_t N, int64_t W, int64_t* d_counts,
                                  int64_t* d_offsets, int32_t* d_triples, int64_t capacity, int64_t* total) {
  if (!ctx) return GNX_EINVAL;
  int rc = label_runs_check(ctx, d_labels, ldl, N, W, d_counts, d_offsets, d_triples, capacity, total);
  if (rc != GNX_OK) return rc;
  GNX_BIND_DEVICE(ctx);
  *total = 0;
  if (N == 0) {
    HIPCHK(ctx, hipMemsetAsync(d_offsets, 0, sizeof(int64_t), ctx->stream));
    return GNX_OK;
  }
  if ((rc = runs_count(ctx, d_labels, ldl, N, W, d_counts, d_offsets, total)) != GNX_OK) return rc;
  if (*total > capacity) return too_small(ctx, *total, capacity);
  if (*total == 0) return GNX_OK;
  return runs_fill(ctx, d_labels, ldl, N, W, d_offsets, d_triples);
}

extern "C" int gnx_label_runs(gnx_ctx* ctx, const int32_t* labels, int64_t ldl, int64_t N, int64_t W, int64_t* counts, int64_t* offsets,
                              int32_t* triples, int64_t capacity, int64_t* total) {
  if (!ctx) return GNX_EINVAL;
  int rc = label_runs_check(ctx, labels, ldl, N, W, counts, offsets, triples, capacity, total);
  if (rc != GNX_OK) return rc;
  GNX_BIND_DEVICE(ctx);
  *total = 0;
  offsets[0] = 0;
  if (N == 0) return GNX_OK;
  hipStream_t s = ctx->stream;
  const size_t bl = ((size_t)(N - 1) * (size_t)ldl + (size_t)W) * sizeof(int32_t);  // the last row ends after its W labels
  const size_t bc = (size_t)N * sizeof(int64_t), bo = (size_t)(N + 1) * sizeof(int64_t);
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_lab, bl + 64)) != GNX_OK) return rc;
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_misc, bc + bo + 64)) != GNX_OK) return rc;
  int32_t* d_lab = (int32_t*)ctx->ws_lab.p;
  int64_t* d_counts = (int64_t*)ctx->ws_misc.p;
  int64_t* d_off = d_counts + N;
  if (bl > 0) HIPCHK(ctx, hipMemcpyAsync(d_lab, labels, bl, hipMemcpyHostToDevice, s));
  if ((rc = runs_count(ctx, d_lab, ldl, N, W, d_counts, d_off, total)) != GNX_OK) return rc;
  HIPCHK(ctx, hipMemcpyAsync(counts, d_counts, bc, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipMemcpyAsync(offsets, d_off, bo, hipMemcpyDeviceToHost, s));
  if (*total > capacity) {
    HIPCHK(ctx, hipStreamSynchronize(s));
    return too_small(ctx, *total, capacity);
  }
  if (*total > 0) {
    const size_t bt = (size_t)*total * 3 * sizeof(int32_t);
    if ((rc = gnx_ws_reserve(ctx, ctx->ws_p32, bt + 64)) != GNX_OK) return rc;
    if ((rc = runs_fill(ctx, d_lab, ldl, N, W, d_off, (int32_t*)ctx->ws_p32.p)) != GNX_OK) return rc;
    HIPCHK(ctx, hipMemcpyAsync(triples, ctx->ws_p32.p, bt, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(ctx, hipStreamSynchronize(s));
  return GNX_OK;
}
