// summary/k_ancestry_assoc.hip — the sufficient statistics of the ancestry-specific association model (Tractor) in one fused pass over
// X and the labels: the per-individual dosage / hapcount matrices of k_allele_counts.hip are never materialised.
//
// Inputs as gnx_ancestry_dosage takes them (rows int8 or 2-bit, labels (N, W) int32, win(c) = min(c / M, W - 1)), plus per individual
// i (rows 2 i, 2 i + 1) a phenotype y[i], covariates Z[i, :K] (row-major float64) and a byte use[i].  h[i, a] / d[i, a] at SNP c are
// hapcount / dosage of ancestry a.  Individual i takes part at window k when use[i] != 0, y[i] and Z[i, :] are finite and both labels
// at k lie in [0, A) (labels are only compared, never used as an index before that test).
//
// k_ancestry_assoc_prep: one thread per individual: part[i] (takes part, as far as y, Z and use say) and zy[i] = (Z[i, :K], y[i]).
// k_ancestry_assoc_window: ONE workgroup per window of the range; U = [Z, h_0 .. h_{A-2}, y] (P + 1 = K + A columns): the Gram matrix
//   U^T U ((P + 1)^2 float64: R^T R, R^T y and y^T y for R = [Z, h_0 .. h_{A-2}]), n and sum_i h[i, a] for every a < A (int32), and the
//   count of labels outside [0, A) among ALL rows of the window.  A thread owns whole entries and walks the individuals.
// k_ancestry_assoc_snp<KIND>: ONE wave per tile of TC <= 64 adjacent SNPs of [c0, c1), lane = SNP; the wave walks ALL individuals, so
//   a (SNP, statistic) has one owner and leaves with a plain store: no atomics, nothing to zero first.  The accumulators live in LDS,
//   [statistic][TC lanes] (a lane only touches its own column: no atomics; where the tile lies in one window the ancestry is the same in
//   every lane and the access is conflict-free).  TC is the largest power of two with TC * (bytes of one SNP's block) <= 64 KiB.
//   Per SNP: float64 [A][K + 1]: D^T Z and, in column K, D^T y; int32: D^T D (upper triangle, row-major: (a, b >= a)), D^T H
//   ([A][A - 1]), sum d [A], n_miss (missing calls on the haplotypes of participating individuals).  An individual touches at most two
//   ancestries: one diagonal square, or two diagonals and one cross term.
//
// SUMMATION ORDER (float64; the integers are exact).  Every float64 sum runs over the individuals in ascending i, one term per
// individual: d[i, a] * zy[i, k] (the SNP blocks; d is 0, 1 or 2, so the product is exact) or u[i, p] * u[i, q] (the window block), each
// rounded once, added to the running sum, no fused multiply-add.  Individuals that do not take part and zero terms are skipped, which
// leaves the sum unchanged.  The order is a function of N alone: not of the grid, of TC, of [c0, c1) or of the row form; nor of the
// file path's batches (accumulate: a later batch of individuals loads the blocks so far and goes on with the same running sums).
//
// The VALU form was kept: a wave's work per (individual, SNP) is dominated by the LDS read-modify-write of the rows the individual's
// two ancestries select, which the float64 matrix cores would not remove.
// No per-thread array is indexed at run time; no scratch.
#include "gnx_summary_host.h"

namespace {

constexpr int AS_THREADS = 64;
constexpr int AS_WIN_THREADS = 256;
constexpr size_t AS_LDS_BYTES = 64 * 1024;
constexpr int AS_MAX_A = GNX_ALLELE_MAX_A;
constexpr int AS_MAX_K = GNX_ASSOC_MAX_K;

// the blocks' sizes: the only definition of the layout (the header states it)
struct AsLayout {
  int K1, NF, oDH, oSD, oMS, NI, P1, NWF, NWI;
  __host__ __device__ AsLayout(int A, int K) {
    K1 = K + 1;
    NF = A * K1;
    oDH = A * (A + 1) / 2;
    oSD = oDH + A * (A - 1);
    oMS = oSD + A;
    NI = oMS + 1;
    P1 = K + A;
    NWF = P1 * P1;
    NWI = 1 + A;
  }
};

__global__ __launch_bounds__(256) void k_ancestry_assoc_prep(const double* __restrict__ y, const double* __restrict__ Z, const uint8_t* __restrict__ use,
                                                             int64_t n_ind, int K, double* __restrict__ zy, uint8_t* __restrict__ part) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_ind) return;
  const int K1 = K + 1;
  const double yi = y[i];
  bool ok = (use == nullptr || use[i] != 0) && isfinite(yi);
  for (int k = 0; k < K; ++k) {
    const double z = Z[i * K + k];
    ok = ok && isfinite(z);
    zy[i * K1 + k] = z;
  }
  zy[i * K1 + K] = yi;
  part[i] = ok ? 1 : 0;
}

__global__ __launch_bounds__(AS_WIN_THREADS) void k_ancestry_assoc_window(const int32_t* __restrict__ lab, int64_t ldl, int64_t n_ind, int A, int K,
                                                                          int64_t w0, const double* __restrict__ zy,
                                                                          const uint8_t* __restrict__ part, int accumulate,
                                                                          double* __restrict__ out_f, int32_t* __restrict__ out_i,
                                                                          unsigned long long* __restrict__ bad) {
  const AsLayout L(A, K);
  const int64_t w = w0 + blockIdx.x;
  const int32_t* lw = lab + w;
  for (int e = threadIdx.x; e < L.NWF + L.NWI; e += AS_WIN_THREADS) {
    if (e < L.NWF) {
      const int p = e / L.P1, q = e - p * L.P1;
      double acc = accumulate ? out_f[(int64_t)blockIdx.x * L.NWF + e] : 0.0;   // a later batch of individuals goes on from the sum so far
      for (int64_t i = 0; i < n_ind; ++i) {
        if (!part[i]) continue;
        const int32_t la = lw[(2 * i) * ldl], lb = lw[(2 * i + 1) * ldl];
        if (la < 0 || la >= A || lb < 0 || lb >= A) continue;
        const double up = p < K ? zy[i * L.K1 + p] : p == L.P1 - 1 ? zy[i * L.K1 + K] : (double)((la == p - K) + (lb == p - K));
        const double uq = q < K ? zy[i * L.K1 + q] : q == L.P1 - 1 ? zy[i * L.K1 + K] : (double)((la == q - K) + (lb == q - K));
        acc += up * uq;
      }
      out_f[(int64_t)blockIdx.x * L.NWF + e] = acc;
    } else {
      const int j = e - L.NWF;     // 0: n (and the labels out of range), 1 + a: sum of h[:, a]
      int32_t acc = accumulate ? out_i[(int64_t)blockIdx.x * L.NWI + j] : 0;
      unsigned long long nbad = 0;
      for (int64_t i = 0; i < n_ind; ++i) {
        const int32_t la = lw[(2 * i) * ldl], lb = lw[(2 * i + 1) * ldl];
        const bool oa = la >= 0 && la < A, ob = lb >= 0 && lb < A;
        nbad += (oa ? 0 : 1) + (ob ? 0 : 1);
        if (!part[i] || !oa || !ob) continue;
        acc += j == 0 ? 1 : (la == j - 1) + (lb == j - 1);
      }
      out_i[(int64_t)blockIdx.x * L.NWI + j] = acc;
      if (j == 0 && nbad) atomicAdd(bad, nbad);
    }
  }
}

template <int KIND>
__global__ __launch_bounds__(AS_THREADS) void k_ancestry_assoc_snp(const uint8_t* __restrict__ rows, int64_t ld, const int32_t* __restrict__ lab,
                                                                   int64_t ldl, int64_t n_ind, int64_t M, int64_t W, int A, int K, int64_t c0,
                                                                   int64_t c1, int TC, const double* __restrict__ zy,
                                                                   const uint8_t* __restrict__ part, int accumulate,
                                                                   double* __restrict__ out_f, int32_t* __restrict__ out_i) {
  extern __shared__ double as_lds[];   // [NF][TC] float64, then [NI][TC] int32
  const AsLayout L(A, K);
  double* accF = as_lds;
  int32_t* accI = reinterpret_cast<int32_t*>(as_lds + (size_t)L.NF * TC);
  const int lane = threadIdx.x;
  const int64_t cb = c0 + (int64_t)blockIdx.x * TC;
  const int ncols = (int)((c1 - cb < TC) ? c1 - cb : TC);     // >= 1 by the grid
  double* of = out_f + (cb - c0) * L.NF;
  int32_t* oi = out_i + (cb - c0) * L.NI;
  for (int e = lane; e < L.NF * TC; e += AS_THREADS) accF[e] = 0.0;
  for (int e = lane; e < L.NI * TC; e += AS_THREADS) accI[e] = 0;
  __syncthreads();
  if (accumulate) {   // a later batch of individuals: go on from the blocks so far (the running sums continue: the order stays ascending i)
    for (int e = lane; e < ncols * L.NF; e += AS_THREADS) {
      const int col = e / L.NF, s = e - col * L.NF;
      accF[s * TC + col] = of[e];
    }
    for (int e = lane; e < ncols * L.NI; e += AS_THREADS) {
      const int col = e / L.NI, s = e - col * L.NI;
      accI[s * TC + col] = oi[e];
    }
    __syncthreads();
  }
  if (lane < ncols) {
    const int64_t c = cb + lane;
    const int64_t w = (c / M < W - 1) ? c / M : W - 1;
    const int32_t* lw = lab + w;
    const int Am1 = A - 1;
    int32_t miss = accI[L.oMS * TC + lane];
    for (int64_t i = 0; i < n_ind; ++i) {
      if (!part[i]) continue;
      const int32_t la = lw[(2 * i) * ldl], lb = lw[(2 * i + 1) * ldl];
      const uint32_t ca = as_code<KIND>(rows + (2 * i) * ld, c), cbv = as_code<KIND>(rows + (2 * i + 1) * ld, c);
      if (la < 0 || la >= A || lb < 0 || lb >= A) continue;
      const int xa = ca == 1u, xb = cbv == 1u;
      miss += (ca > 1u) + (cbv > 1u);
      if (!(xa | xb)) continue;
      const double* z = zy + i * L.K1;
      const int daa = la * A - la * (la - 1) / 2, dbb = lb * A - lb * (lb - 1) / 2;   // the diagonal entries (a, a) of the triangle
      if (la == lb) {
        const int d = xa + xb;
        accI[daa * TC + lane] += d * d;
        accI[(L.oSD + la) * TC + lane] += d;
        if (la < Am1) accI[(L.oDH + la * Am1 + la) * TC + lane] += 2 * d;
        const double dd = (double)d;
        for (int k = 0; k < L.K1; ++k) accF[(la * L.K1 + k) * TC + lane] += dd * z[k];
      } else {
        if (xa) {
          accI[daa * TC + lane] += 1;
          accI[(L.oSD + la) * TC + lane] += 1;
          if (la < Am1) accI[(L.oDH + la * Am1 + la) * TC + lane] += 1;
          if (lb < Am1) accI[(L.oDH + la * Am1 + lb) * TC + lane] += 1;
          for (int k = 0; k < L.K1; ++k) accF[(la * L.K1 + k) * TC + lane] += z[k];
        }
        if (xb) {
          accI[dbb * TC + lane] += 1;
          accI[(L.oSD + lb) * TC + lane] += 1;
          if (lb < Am1) accI[(L.oDH + lb * Am1 + lb) * TC + lane] += 1;
          if (la < Am1) accI[(L.oDH + lb * Am1 + la) * TC + lane] += 1;
          for (int k = 0; k < L.K1; ++k) accF[(lb * L.K1 + k) * TC + lane] += z[k];
        }
        if (xa & xb) {
          const int lo = la < lb ? la : lb, hi = la < lb ? lb : la;
          accI[(lo * A - lo * (lo - 1) / 2 + (hi - lo)) * TC + lane] += 1;
        }
      }
    }
    accI[L.oMS * TC + lane] = miss;
  }
  __syncthreads();
  // the tile's blocks leave SNP-major: adjacent lanes write adjacent words
  for (int e = lane; e < ncols * L.NF; e += AS_THREADS) {
    const int col = e / L.NF, s = e - col * L.NF;
    of[e] = accF[s * TC + col];
  }
  for (int e = lane; e < ncols * L.NI; e += AS_THREADS) {
    const int col = e / L.NI, s = e - col * L.NI;
    oi[e] = accI[s * TC + col];
  }
}

// the largest power of two <= 64 whose tile of blocks fits AS_LDS_BYTES (>= 4 at A = 32, K = 16)
int as_tile_cols(const AsLayout& L) {
  const size_t per = (size_t)L.NF * 8 + (size_t)L.NI * 4;
  int tc = AS_THREADS;
  while (tc > 1 && (size_t)tc * per > AS_LDS_BYTES) tc >>= 1;
  return tc;
}

const char* const AS_TAIL = "an individual with such a label takes no part at that window";

// every refusal before the launch; GNX_OK or the code.  built: the rows are built by this call (the file path's form)
int assoc_check(gnx_ctx* ctx, bool built, const void* rows, int row_kind, int64_t ld_rows, const void* labels, int64_t ld_labels, int64_t N, int64_t C,
                int64_t M, int64_t W, int32_t A, const void* y, const void* Z, int32_t K, int32_t min_ac, int64_t c0, int64_t c1, const void* snp_f64,
                const void* snp_i32, const void* win_f64, const void* win_i32) {
  const std::string w("ancestry_assoc_stats");
  const int rc = gnx_sum_geometry_check(ctx, "ancestry_assoc_stats", GNX_SUM_N_EVEN | GNX_SUM_OWN_NULLS, rows, row_kind, ld_rows, labels, ld_labels, N, C,
                                        M, W, A);
  if (rc != GNX_OK) return rc;
  if (K < 1) return gnx_fail(ctx, GNX_EINVAL, w + ": need K >= 1 covariates (the caller supplies the intercept column)");
  if (min_ac < 1) return gnx_fail(ctx, GNX_EINVAL, w + ": need min_ac >= 1");
  if (c0 < 0 || c1 > C || c0 >= c1) return gnx_fail(ctx, GNX_EINVAL, w + ": need 0 <= c0 < c1 <= C");
  if ((!built && !rows) || !labels || !y || !Z || !snp_f64 || !snp_i32 || !win_f64 || !win_i32)
    return gnx_fail(ctx, GNX_EINVAL, w + ": a null pointer (only use and n_bad may be NULL)");
  if (A > AS_MAX_A) return gnx_fail(ctx, GNX_EUNSUPPORTED, w + ": A = " + std::to_string(A) + " ancestries, at most " + std::to_string(AS_MAX_A));
  if (K > AS_MAX_K) return gnx_fail(ctx, GNX_EUNSUPPORTED, w + ": K = " + std::to_string(K) + " covariates, at most " + std::to_string(AS_MAX_K));
  if (N > ((int64_t)1 << 28)) return gnx_fail(ctx, GNX_EUNSUPPORTED, w + ": N must not exceed 2^28 (the integer blocks are int32)");
  return GNX_OK;
}

// the window and SNP kernels over n_ind individuals (rows, labels, zy and part of THOSE individuals); accumulate: the outputs hold the
// blocks of the individuals before them.  Arguments checked by the caller.
hipError_t assoc_launch(const void* d_rows, int row_kind, int64_t ld_rows, const int32_t* d_labels, int64_t ld_labels, int64_t n_ind, int64_t M,
                        int64_t W, int32_t A, int32_t K, int64_t c0, int64_t c1, const double* zy, const uint8_t* part, int accumulate,
                        double* d_snp_f64, int32_t* d_snp_i32, double* d_win_f64, int32_t* d_win_i32, unsigned long long* d_bad, hipStream_t s) {
  const AsLayout L(A, K);
  const int64_t nc = c1 - c0, w0 = as_win(c0, M, W), nw = as_win(c1 - 1, M, W) - w0 + 1;
  hipLaunchKernelGGL(k_ancestry_assoc_window, dim3((unsigned)nw), dim3(AS_WIN_THREADS), 0, s, d_labels, ld_labels, n_ind, (int)A, (int)K, w0, zy, part,
                     accumulate, d_win_f64, d_win_i32, d_bad);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int tc = as_tile_cols(L);
  const size_t lds = (size_t)tc * ((size_t)L.NF * 8 + (size_t)L.NI * 4);
  const dim3 grid((unsigned)((nc + tc - 1) / tc));
  const uint8_t* rows = (const uint8_t*)d_rows;
  if (row_kind == GNX_ROWS_PACKED2)
    hipLaunchKernelGGL(k_ancestry_assoc_snp<GNX_ROWS_PACKED2>, grid, dim3(AS_THREADS), lds, s, rows, ld_rows, d_labels, ld_labels, n_ind, M, W, (int)A,
                       (int)K, c0, c1, tc, zy, part, accumulate, d_snp_f64, d_snp_i32);
  else
    hipLaunchKernelGGL(k_ancestry_assoc_snp<GNX_ROWS_INT8>, grid, dim3(AS_THREADS), lds, s, rows, ld_rows, d_labels, ld_labels, n_ind, M, W, (int)A,
                       (int)K, c0, c1, tc, zy, part, accumulate, d_snp_f64, d_snp_i32);
  return hipGetLastError();
}

// the workspace of one call: zy | part in ws_p64, filled from DEVICE y, Z and use, and the zeroed counter of labels out of range
struct AsWork {
  double* zy;
  uint8_t* part;
  unsigned long long* d_bad;
};

int assoc_work(gnx_ctx* ctx, int64_t n_ind, int32_t K, const double* d_y, const double* d_Z, const uint8_t* d_use, AsWork* wk, hipStream_t s) {
  int rc;
  if ((rc = gnx_sum_zy_part(ctx, n_ind, K, &wk->zy, &wk->part)) != GNX_OK) return rc;
  if ((rc = gnx_sum_bad_counter(ctx, 1, &wk->d_bad, s)) != GNX_OK) return rc;
  if (n_ind > 0) {
    hipLaunchKernelGGL(k_ancestry_assoc_prep, dim3((unsigned)((n_ind + 255) / 256)), dim3(256), 0, s, d_y, d_Z, d_use, n_ind, (int)K, wk->zy, wk->part);
    HIPCHK(ctx, hipGetLastError());
  }
  return GNX_OK;
}

// host outputs of one call: the float64 blocks in ws_b64, the int32 blocks in ws_b32
struct AsOut {
  size_t sf, si, wf, wi;
  double *d_sf, *d_wf;
  int32_t *d_si, *d_wi;
};

int assoc_out(gnx_ctx* ctx, int32_t A, int32_t K, int64_t M, int64_t W, int64_t c0, int64_t c1, AsOut* o) {
  const AsLayout L(A, K);
  const size_t nc = (size_t)(c1 - c0), nw = (size_t)(as_win(c1 - 1, M, W) - as_win(c0, M, W) + 1);
  const auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  o->sf = nc * L.NF * 8, o->si = nc * L.NI * 4, o->wf = nw * L.NWF * 8, o->wi = nw * L.NWI * 4;
  int rc;
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_b64, up(o->sf) + o->wf + 64)) != GNX_OK) return rc;
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_b32, up(o->si) + o->wi + 64)) != GNX_OK) return rc;
  o->d_sf = (double*)ctx->ws_b64.p, o->d_wf = (double*)((char*)ctx->ws_b64.p + up(o->sf));
  o->d_si = (int32_t*)ctx->ws_b32.p, o->d_wi = (int32_t*)((char*)ctx->ws_b32.p + up(o->si));
  return GNX_OK;
}

// the four blocks -> the host; synchronises the stream
int assoc_copy_out(gnx_ctx* ctx, const AsOut& o, double* snp_f64, int32_t* snp_i32, double* win_f64, int32_t* win_i32, hipStream_t s) {
  HIPCHK(ctx, hipMemcpyAsync(snp_f64, o.d_sf, o.sf, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipMemcpyAsync(snp_i32, o.d_si, o.si, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipMemcpyAsync(win_f64, o.d_wf, o.wf, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipMemcpyAsync(win_i32, o.d_wi, o.wi, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  return GNX_OK;
}

}  // namespace

extern "C" int gnx_ancestry_assoc_stats_dev(gnx_ctx* ctx, const void* d_rows, int row_kind, int64_t ld_rows, const int32_t* d_labels, int64_t ld_labels,
                                            int64_t N, int64_t C, int64_t M, int64_t W, int32_t A, const double* d_y, const double* d_Z, int32_t K,
                                            const uint8_t* d_use, int32_t min_ac, int64_t c0, int64_t c1, double* d_snp_f64, int32_t* d_snp_i32,
                                            double* d_win_f64, int32_t* d_win_i32, int64_t* n_bad) {
  if (!ctx) return GNX_EINVAL;
  int rc = assoc_check(ctx, false, d_rows, row_kind, ld_rows, d_labels, ld_labels, N, C, M, W, A, d_y, d_Z, K, min_ac, c0, c1, d_snp_f64, d_snp_i32,
                       d_win_f64, d_win_i32);
  if (rc != GNX_OK) return rc;
  GNX_BIND_DEVICE(ctx);
  hipStream_t s = ctx->stream;
  AsWork wk;
  if ((rc = assoc_work(ctx, N / 2, K, d_y, d_Z, d_use, &wk, s)) != GNX_OK) return rc;
  HIPCHK(ctx, assoc_launch(d_rows, row_kind, ld_rows, d_labels, ld_labels, N / 2, M, W, A, K, c0, c1, wk.zy, wk.part, 0, d_snp_f64, d_snp_i32, d_win_f64,
                           d_win_i32, wk.d_bad, s));
  return gnx_sum_read_verdict(ctx, "ancestry_assoc_stats", wk.d_bad, A, AS_TAIL, n_bad, s);
}

extern "C" int gnx_ancestry_assoc_stats(gnx_ctx* ctx, const int8_t* X, int64_t ld_rows, const int32_t* labels, int64_t ld_labels, int64_t N, int64_t C,
                                        int64_t M, int64_t W, int32_t A, const double* y, const double* Z, int32_t K, const uint8_t* use,
                                        int32_t min_ac, int64_t c0, int64_t c1, double* snp_f64, int32_t* snp_i32, double* win_f64, int32_t* win_i32,
                                        int64_t* n_bad) {
  if (!ctx) return GNX_EINVAL;
  int rc = assoc_check(ctx, false, X, GNX_ROWS_INT8, ld_rows, labels, ld_labels, N, C, M, W, A, y, Z, K, min_ac, c0, c1, snp_f64, snp_i32, win_f64,
                       win_i32);
  if (rc != GNX_OK) return rc;
  GNX_BIND_DEVICE(ctx);
  hipStream_t s = ctx->stream;
  // inputs: rows -> ws_xu, labels -> ws_lab, y | Z | use -> ws_scale; outputs: float64 blocks in ws_b64, int32 blocks in ws_b32
  gnx_sum_pheno ph;
  AsOut o;
  if ((rc = gnx_sum_stage_rows_labels(ctx, X, GNX_ROWS_INT8, ld_rows, labels, ld_labels, N, C, W, s)) != GNX_OK) return rc;
  if ((rc = gnx_sum_stage_pheno(ctx, y, Z, K, use, N / 2, &ph, s)) != GNX_OK) return rc;
  if ((rc = assoc_out(ctx, A, K, M, W, c0, c1, &o)) != GNX_OK) return rc;
  rc = gnx_ancestry_assoc_stats_dev(ctx, ctx->ws_xu.p, GNX_ROWS_INT8, ld_rows, (const int32_t*)ctx->ws_lab.p, ld_labels, N, C, M, W, A, ph.d_y, ph.d_Z, K,
                                    ph.d_use, min_ac, c0, c1, o.d_sf, o.d_si, o.d_wf, o.d_wi, n_bad);
  if (rc != GNX_OK && rc != GNX_EINVAL) return rc;
  // (GNX_EINVAL after the launch = labels out of range: the other values stand and are handed over)
  const std::string msg = ctx->err;
  const int rc2 = assoc_copy_out(ctx, o, snp_f64, snp_i32, win_f64, win_i32, s);
  if (rc2 != GNX_OK) return rc2;
  ctx->err = msg;
  return rc;
}

// The file path's form: the packed rows of gnx_infer_gt2's batches (gnx_summary_host.h: the staging, column map, row pitch and batch
// size), reduced against the caller's labels batch by batch.  A batch holds whole individuals in ascending order and goes on from the
// blocks of the batches before it (accumulate), so every running sum is the one a single launch makes: the blocks do not depend on the
// batch size.
extern "C" int gnx_ancestry_assoc_stats_gt2(gnx_model* m, const uint8_t* G, int64_t V, int64_t ldg, int64_t N, const int32_t* src,
                                            const int32_t* labels, const double* y, const double* Z, int32_t K, const uint8_t* use, int32_t min_ac,
                                            int64_t c0, int64_t c1, double* snp_f64, int32_t* snp_i32, double* win_f64, int32_t* win_i32,
                                            int64_t* n_bad) {
  if (!m) return GNX_EINVAL;
  gnx_ctx* ctx = m->ctx;
  const int64_t C = m->info.C, M = m->info.M, W = m->info.W;
  const int32_t A = m->info.A;
  int rc = gnx_sum_gt2_args(ctx, "ancestry_assoc_stats_gt2", G, V, ldg, N, src);
  if (rc != GNX_OK) return rc;
  if ((rc = assoc_check(ctx, true, nullptr, GNX_ROWS_PACKED2, (C + 3) / 4, labels, W, N, C, M, W, A, y, Z, K, min_ac, c0, c1, snp_f64, snp_i32, win_f64,
                        win_i32)) != GNX_OK)
    return rc;
  if ((rc = gnx_sum_check_src(ctx, "ancestry_assoc_stats_gt2", src, C, V)) != GNX_OK) return rc;
  GNX_BIND_DEVICE(ctx);
  hipStream_t s = ctx->stream;
  gnx_sum_gt2 st;
  gnx_sum_pheno ph;
  AsWork wk;
  AsOut o;
  if ((rc = gnx_sum_gt2_stage(ctx, G, V, ldg, N, src, labels, C, W, true, &st, s)) != GNX_OK) return rc;
  if ((rc = gnx_sum_stage_pheno(ctx, y, Z, K, use, N / 2, &ph, s)) != GNX_OK) return rc;
  if ((rc = assoc_work(ctx, N / 2, K, ph.d_y, ph.d_Z, ph.d_use, &wk, s)) != GNX_OK) return rc;
  if ((rc = assoc_out(ctx, A, K, M, W, c0, c1, &o)) != GNX_OK) return rc;
  if (N == 0)   // no individuals: the blocks of nobody
    HIPCHK(ctx, assoc_launch(ctx->ws_xu.p, GNX_ROWS_PACKED2, st.ldp, st.d_lab, W, 0, M, W, A, K, c0, c1, wk.zy, wk.part, 0, o.d_sf, o.d_si, o.d_wf, o.d_wi,
                             wk.d_bad, s));
  for (int64_t n0 = 0; n0 < N; n0 += st.nb) {   // (nb is a multiple of 4: a batch holds whole individuals)
    const int64_t n = std::min(st.nb, N - n0);
    HIPCHK(ctx, gnx_sum_gt2_batch(st, n0, n, C, ctx->ws_xu.p, s));
    HIPCHK(ctx, assoc_launch(ctx->ws_xu.p, GNX_ROWS_PACKED2, st.ldp, st.d_lab + n0 * W, W, n / 2, M, W, A, K, c0, c1, wk.zy + (n0 / 2) * (K + 1),
                             wk.part + n0 / 2, n0 > 0, o.d_sf, o.d_si, o.d_wf, o.d_wi, wk.d_bad, s));
  }
  unsigned long long h_bad = 0;
  HIPCHK(ctx, hipMemcpyAsync(&h_bad, wk.d_bad, sizeof h_bad, hipMemcpyDeviceToHost, s));
  if ((rc = assoc_copy_out(ctx, o, snp_f64, snp_i32, win_f64, win_i32, s)) != GNX_OK) return rc;
  return gnx_sum_label_verdict(ctx, "ancestry_assoc_stats_gt2", h_bad, A, AS_TAIL, n_bad);
}
