// summary/k_ancestry_assoc_traits.hip — the trait-dependent statistics of the ancestry-specific association model (Tractor) for T
// quantitative traits at once: D^T Y per SNP on the float64 matrix cores, [Z, H]^T Y and diag(Y^T Y) per window.  Everything that
// does not depend on the trait (the integer blocks, D^T Z, the Gram matrix of [Z, H]) is k_ancestry_assoc.hip's, unchanged: the caller
// runs that entry with use & (all of Y[i, :] finite) and a zero phenotype (include/gnomix_hip.h states the contract).
//
// Inputs as gnx_ancestry_assoc_stats takes them, with Y (N / 2, T) float64 (row stride ldy) in place of y.  Individual i takes part at
// window k when use[i] != 0, Z[i, :] is finite, EVERY entry of Y[i, :] is finite and both labels at k lie in [0, A) (labels are only
// compared, never used as an index).  ldt = T rounded up to a multiple of 16; n_pad = N / 2 rounded up to a multiple of 4.
//
// k_ancestry_assoc_traits_prep: one thread per individual i < n_pad: part[i] (takes part, as far as use, Z and Y say; 0 for i >= N / 2)
//   and the cleaned copy Yc (n_pad, ldt): Yc[i, t] = Y[i, t] where part[i] and t < T, else +0.0.  No NaN or infinity reaches the matrix
//   pipe (0 * inf is NaN); a bad label at a window is a zero A operand instead.
// k_ancestry_assoc_traits_snp<KIND, AG, NT>: ONE wave per (tile of 16 adjacent SNPs of [c0, c1), group of AG ancestries, group of NT
//   trait tiles of 16).  v_mfma_f64_16x16x4_f64 with M = the 16 SNPs, N = 16 traits, K = 4 consecutive individuals i0 .. i0 + 3:
//     A operand of lane l: d[i0 + (l >> 4)][cb + (l & 15)][a] in {0, 1, 2}, built from the lane's own field of both haplotype rows and
//       the two labels of that SNP'S OWN window (a tile may straddle a boundary); 0 where the individual takes no part there;
//     B operand of lane l: Yc[i0 + (l >> 4)][16 tt + (l & 15)], one 128-byte row segment per individual, shared by the AG ancestries;
//     C / D: column (trait) = l & 15, row (SNP) = (l >> 4) + 4 reg.
//   The wave walks ALL individuals in ascending groups of 4 with the AG x NT accumulators (8 VGPRs each: 256 at AG x NT = 32) in
//   registers, so an output has one owner and leaves with a plain store: no atomics, nothing to zero first.  A wave carries AG = 4
//   ancestries at once where A <= 4, else AG = 8; with A > AG the individuals are walked again per ancestry group (grid.y).  Ancestries
//   >= A and trait tiles >= ldt / 16 of the last groups issue no MFMA (wave-uniform branches; the registers are indexed statically).
//   The next group's bytes, labels and Yc segments are loaded before the current group's MFMAs are issued.
// k_ancestry_assoc_traits_window: a thread owns one entry (p, t) of a window's [Z, h_0 .. h_{A-2}]^T Y (p < K + A - 1) or of diag(Y^T Y)
//   and walks the participants in ascending i: acc += u[i, p] * Yc[i, t], the product rounded once, no fused multiply-add.  Block
//   (window, 0) also counts the labels outside [0, A) among ALL rows of the window.
//
// SUMMATION ORDER.  Products d * y with d in {0, 1, 2} are exact.  D^T Y: the accumulator runs over the individuals in ascending
// groups of 4 from +0.0; the order of the four terms inside one MFMA is the hardware's.  Window blocks: ascending i, one term per
// participant.  Either is a function of N and the data alone: not of the grid, of AG or NT, of [c0, c1) or of the row form; nor of the
// file path's batches, which are cut at whole groups of 4 individuals and go on from the accumulators so far (accumulate).
// No per-thread array is indexed at run time; no scratch.
#include "gnx_summary_host.h"

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int AT_WIN_THREADS = 256;
constexpr int AT_MAX_A = GNX_ALLELE_MAX_A;
constexpr int AT_MAX_K = GNX_ASSOC_MAX_K;
constexpr int AT_MAX_T = GNX_ASSOC_MAX_T;

__host__ __device__ inline int at_ldt(int T) { return (T + 15) / 16 * 16; }
inline int64_t at_pad4(int64_t n) { return (n + 3) / 4 * 4; }

__global__ __launch_bounds__(256) void k_ancestry_assoc_traits_prep(const double* __restrict__ Y, int64_t ldy, int T, const double* __restrict__ Z,
                                                                    const uint8_t* __restrict__ use, int64_t n_ind, int64_t n_pad, int K, int ldt,
                                                                    double* __restrict__ Yc, uint8_t* __restrict__ part) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_pad) return;
  bool ok = i < n_ind && (use == nullptr || use[i] != 0);
  if (ok) {
    for (int k = 0; k < K; ++k) ok = ok && isfinite(Z[i * K + k]);
    for (int t = 0; t < T; ++t) ok = ok && isfinite(Y[i * ldy + t]);
  }
  double* yc = Yc + i * ldt;
  for (int t = 0; t < ldt; ++t) yc[t] = (ok && t < T) ? Y[i * ldy + t] : 0.0;
  part[i] = ok ? 1 : 0;
}

__global__ __launch_bounds__(AT_WIN_THREADS) void k_ancestry_assoc_traits_window(const int32_t* __restrict__ lab, int64_t ldl, int64_t n_ind, int A, int K,
                                                                                 int64_t w0, const double* __restrict__ Z,
                                                                                 const double* __restrict__ Yc, int ldt,
                                                                                 const uint8_t* __restrict__ part, int accumulate,
                                                                                 double* __restrict__ win_y, double* __restrict__ win_yy,
                                                                                 unsigned long long* __restrict__ bad) {
  const int P = K + A - 1;
  const int32_t* lw = lab + (w0 + blockIdx.x);
  if (blockIdx.y == 0) {   // labels out of range among ALL rows of the window
    unsigned int nbad = 0;
    for (int64_t i = threadIdx.x; i < n_ind; i += AT_WIN_THREADS) {
      const int32_t la = lw[(2 * i) * ldl], lb = lw[(2 * i + 1) * ldl];
      nbad += ((la >= 0 && la < A) ? 0 : 1) + ((lb >= 0 && lb < A) ? 0 : 1);
    }
    if (nbad) atomicAdd(bad, (unsigned long long)nbad);
  }
  const int e = (int)blockIdx.y * AT_WIN_THREADS + (int)threadIdx.x;
  if (e >= (P + 1) * ldt) return;
  const int p = e / ldt, t = e - p * ldt;
  double* dst = p < P ? win_y + ((int64_t)blockIdx.x * P + p) * ldt + t : win_yy + (int64_t)blockIdx.x * ldt + t;
  double acc = accumulate ? *dst : 0.0;   // a later batch of individuals goes on from the sum so far
  for (int64_t i = 0; i < n_ind; ++i) {
    if (!part[i]) continue;
    const int32_t la = lw[(2 * i) * ldl], lb = lw[(2 * i + 1) * ldl];
    if (la < 0 || la >= A || lb < 0 || lb >= A) continue;
    const double yv = Yc[i * ldt + t];
    const double u = p < K ? Z[i * K + p] : p < P ? (double)((la == p - K) + (lb == p - K)) : yv;
    acc += u * yv;
  }
  *dst = acc;
}

// what lane l needs of individual i0 + (l >> 4) at its SNP: both fields, both labels, the participation byte
struct AtRaw {
  int32_t la, lb;
  uint32_t ca, cb;
  uint32_t p;
};

template <int KIND>
__device__ __forceinline__ AtRaw at_load(const uint8_t* __restrict__ rows, int64_t ld, const int32_t* __restrict__ lw, int64_t ldl, int64_t c,
                                         const uint8_t* __restrict__ part, int64_t i, int64_t n_ind) {
  const int64_t ii = i < n_ind ? i : n_ind - 1;   // rows past the last individual repeat it (part is 0 there: n_pad bytes)
  AtRaw r;
  r.p = part[i];
  r.la = lw[(2 * ii) * ldl];
  r.lb = lw[(2 * ii + 1) * ldl];
  r.ca = as_code<KIND>(rows + (2 * ii) * ld, c);
  r.cb = as_code<KIND>(rows + (2 * ii + 1) * ld, c);
  return r;
}

template <int KIND, int AG, int NT>
__global__ __launch_bounds__(64) void k_ancestry_assoc_traits_snp(const uint8_t* __restrict__ rows, int64_t ld, const int32_t* __restrict__ lab,
                                                                  int64_t ldl, int64_t n_ind, int64_t M, int64_t W, int A, int64_t c0, int64_t c1,
                                                                  const double* __restrict__ Yc, int ldt, int n_tg,
                                                                  const uint8_t* __restrict__ part, int accumulate, double* __restrict__ out) {
  const int lane = threadIdx.x;
  const int r16 = lane & 15, kq = lane >> 4;
  const int64_t cb = c0 + (int64_t)blockIdx.x * 16;
  const int tg = (int)blockIdx.y % n_tg, a0 = ((int)blockIdx.y / n_tg) * AG, tt0 = tg * NT, n_tt = ldt / 16;
  // the A operand's SNP of this lane; lanes past c1 repeat the last SNP (their results are never stored)
  const int64_t c = cb + r16 < c1 ? cb + r16 : c1 - 1;
  const int64_t w = (c / M < W - 1) ? c / M : W - 1;
  const int32_t* lw = lab + w;
  // the B operand's column of this lane per trait tile; tiles past the last repeat it (no MFMA is issued for them)
  const double* yb[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) yb[j] = Yc + (size_t)kq * ldt + (size_t)((tt0 + j < n_tt ? tt0 + j : n_tt - 1) * 16 + r16);

  d4 acc[AG][NT];
#pragma unroll
  for (int q = 0; q < AG; ++q)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[q][j] = d4{0.0, 0.0, 0.0, 0.0};
  if (accumulate) {   // a later batch of individuals: go on from the blocks so far
#pragma unroll
    for (int q = 0; q < AG; ++q)
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t cs = cb + kq + 4 * r;
          if (cs < c1 && a0 + q < A && tt0 + j < n_tt) acc[q][j][r] = out[((cs - c0) * A + (a0 + q)) * ldt + (tt0 + j) * 16 + r16];
        }
  }

  if (n_ind > 0) {
    AtRaw nx = at_load<KIND>(rows, ld, lw, ldl, c, part, kq, n_ind);
    double bn[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) bn[j] = yb[j][0];
    for (int64_t i0 = 0; i0 < n_ind; i0 += 4) {
      const AtRaw cur = nx;
      double b[NT];
#pragma unroll
      for (int j = 0; j < NT; ++j) b[j] = bn[j];
      if (i0 + 4 < n_ind) {   // the next group of 4, in flight while this one's MFMAs issue
        nx = at_load<KIND>(rows, ld, lw, ldl, c, part, i0 + 4 + kq, n_ind);
#pragma unroll
        for (int j = 0; j < NT; ++j) bn[j] = yb[j][(size_t)(i0 + 4) * ldt];
      }
      const bool takes = cur.p != 0 && cur.la >= 0 && cur.la < A && cur.lb >= 0 && cur.lb < A;
      const int xa = (takes && cur.ca == 1u) ? 1 : 0, xb = (takes && cur.cb == 1u) ? 1 : 0;
#pragma unroll
      for (int q = 0; q < AG; ++q) {
        if (a0 + q < A) {
          const double d = (double)((cur.la == a0 + q ? xa : 0) + (cur.lb == a0 + q ? xb : 0));
#pragma unroll
          for (int j = 0; j < NT; ++j)
            if (tt0 + j < n_tt) acc[q][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(d, b[j], acc[q][j], 0, 0, 0);
        }
      }
    }
  }

  // the accumulator layout: trait = lane & 15, SNP = (lane >> 4) + 4 reg: 16 lanes write one 128-byte segment of (SNP, ancestry)
#pragma unroll
  for (int q = 0; q < AG; ++q)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t cs = cb + kq + 4 * r;
        if (cs < c1 && a0 + q < A && tt0 + j < n_tt) out[((cs - c0) * A + (a0 + q)) * ldt + (tt0 + j) * 16 + r16] = acc[q][j][r];
      }
}

const char* const AT_TAIL = "an individual with such a label takes no part at that window";
const char* const AT_WHO = "ancestry_assoc_traits";

// every refusal before the launch; GNX_OK or the code.  built: the rows are built by this call (the file path's form)
int traits_check(gnx_ctx* ctx, bool built, const void* rows, int row_kind, int64_t ld_rows, const void* labels, int64_t ld_labels, int64_t N, int64_t C,
                 int64_t M, int64_t W, int32_t A, const void* Y, int64_t ldy, int32_t T, const void* Z, int32_t K, int32_t min_ac, int64_t c0, int64_t c1,
                 const void* snp_y, const void* win_y, const void* win_yy) {
  const std::string w(AT_WHO);
  const int rc = gnx_sum_geometry_check(ctx, AT_WHO, GNX_SUM_N_EVEN | GNX_SUM_OWN_NULLS, rows, row_kind, ld_rows, labels, ld_labels, N, C, M, W, A);
  if (rc != GNX_OK) return rc;
  if (K < 1) return gnx_fail(ctx, GNX_EINVAL, w + ": need K >= 1 covariates (the caller supplies the intercept column)");
  if (T < 1 || ldy < T) return gnx_fail(ctx, GNX_EINVAL, w + ": need T >= 1 traits and a row stride of Y of at least T");
  if (min_ac < 1) return gnx_fail(ctx, GNX_EINVAL, w + ": need min_ac >= 1");
  if (c0 < 0 || c1 > C || c0 >= c1) return gnx_fail(ctx, GNX_EINVAL, w + ": need 0 <= c0 < c1 <= C");
  if ((!built && !rows) || !labels || !Y || !Z || !snp_y || !win_y || !win_yy)
    return gnx_fail(ctx, GNX_EINVAL, w + ": a null pointer (only use and n_bad may be NULL)");
  if (A > AT_MAX_A) return gnx_fail(ctx, GNX_EUNSUPPORTED, w + ": A = " + std::to_string(A) + " ancestries, at most " + std::to_string(AT_MAX_A));
  if (K > AT_MAX_K) return gnx_fail(ctx, GNX_EUNSUPPORTED, w + ": K = " + std::to_string(K) + " covariates, at most " + std::to_string(AT_MAX_K));
  if (T > AT_MAX_T) return gnx_fail(ctx, GNX_EUNSUPPORTED, w + ": T = " + std::to_string(T) + " traits, at most " + std::to_string(AT_MAX_T));
  if (N > ((int64_t)1 << 28)) return gnx_fail(ctx, GNX_EUNSUPPORTED, w + ": N must not exceed 2^28 (as the trait-independent blocks)");
  return GNX_OK;
}

template <int KIND, int AG>
void traits_snp_launch(int nt, dim3 grid, hipStream_t s, const uint8_t* rows, int64_t ld, const int32_t* lab, int64_t ldl, int64_t n_ind, int64_t M,
                       int64_t W, int A, int64_t c0, int64_t c1, const double* Yc, int ldt, int n_tg, const uint8_t* part, int accumulate, double* out) {
  if (nt == 1)
    hipLaunchKernelGGL((k_ancestry_assoc_traits_snp<KIND, AG, 1>), grid, dim3(64), 0, s, rows, ld, lab, ldl, n_ind, M, W, A, c0, c1, Yc, ldt, n_tg, part,
                       accumulate, out);
  else if (nt == 2)
    hipLaunchKernelGGL((k_ancestry_assoc_traits_snp<KIND, AG, 2>), grid, dim3(64), 0, s, rows, ld, lab, ldl, n_ind, M, W, A, c0, c1, Yc, ldt, n_tg, part,
                       accumulate, out);
  else
    hipLaunchKernelGGL((k_ancestry_assoc_traits_snp<KIND, AG, 4>), grid, dim3(64), 0, s, rows, ld, lab, ldl, n_ind, M, W, A, c0, c1, Yc, ldt, n_tg, part,
                       accumulate, out);
}

// the window and SNP kernels over n_ind individuals (rows, labels, Z, Yc and part of THOSE individuals; Yc and part reach to the next
// multiple of 4); accumulate: the outputs hold the blocks of the individuals before them.  Arguments checked by the caller.
hipError_t traits_launch(const void* d_rows, int row_kind, int64_t ld_rows, const int32_t* d_labels, int64_t ld_labels, int64_t n_ind, int64_t M,
                         int64_t W, int32_t A, int32_t K, int32_t T, int64_t c0, int64_t c1, const double* d_Z, const double* Yc, const uint8_t* part,
                         int accumulate, double* d_snp_y, double* d_win_y, double* d_win_yy, unsigned long long* d_bad, hipStream_t s) {
  const int ldt = at_ldt(T), n_tt = ldt / 16;
  const int64_t nc = c1 - c0, w0 = as_win(c0, M, W), nw = as_win(c1 - 1, M, W) - w0 + 1;
  const int entries = (K + A) * ldt;   // (P + 1) ldt <= 48 * 2^16
  hipLaunchKernelGGL(k_ancestry_assoc_traits_window, dim3((unsigned)nw, (unsigned)((entries + AT_WIN_THREADS - 1) / AT_WIN_THREADS)), dim3(AT_WIN_THREADS),
                     0, s, d_labels, ld_labels, n_ind, (int)A, (int)K, w0, d_Z, Yc, ldt, part, accumulate, d_win_y, d_win_yy, d_bad);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int ag = A <= 4 ? 4 : 8, nt = n_tt >= 4 ? 4 : n_tt >= 2 ? 2 : 1;   // (n_tt = 3: two groups of 2)
  const int n_ag = (A + ag - 1) / ag, n_tg = (n_tt + nt - 1) / nt;         // n_ag n_tg <= 4 * 1024 < 65536
  const dim3 grid((unsigned)((nc + 15) / 16), (unsigned)(n_ag * n_tg));
  const uint8_t* rows = (const uint8_t*)d_rows;
  if (row_kind == GNX_ROWS_PACKED2) {
    if (ag == 4) traits_snp_launch<GNX_ROWS_PACKED2, 4>(nt, grid, s, rows, ld_rows, d_labels, ld_labels, n_ind, M, W, A, c0, c1, Yc, ldt, n_tg, part, accumulate, d_snp_y);
    else traits_snp_launch<GNX_ROWS_PACKED2, 8>(nt, grid, s, rows, ld_rows, d_labels, ld_labels, n_ind, M, W, A, c0, c1, Yc, ldt, n_tg, part, accumulate, d_snp_y);
  } else {
    if (ag == 4) traits_snp_launch<GNX_ROWS_INT8, 4>(nt, grid, s, rows, ld_rows, d_labels, ld_labels, n_ind, M, W, A, c0, c1, Yc, ldt, n_tg, part, accumulate, d_snp_y);
    else traits_snp_launch<GNX_ROWS_INT8, 8>(nt, grid, s, rows, ld_rows, d_labels, ld_labels, n_ind, M, W, A, c0, c1, Yc, ldt, n_tg, part, accumulate, d_snp_y);
  }
  return hipGetLastError();
}

// the workspace of one call: Yc | part in ws_p64, filled from DEVICE Y, Z and use, and the zeroed counter of labels out of range
struct AtWork {
  double* Yc;
  uint8_t* part;
  unsigned long long* d_bad;
};

int traits_work(gnx_ctx* ctx, int64_t n_ind, int32_t K, int32_t T, const double* d_Y, int64_t ldy, const double* d_Z, const uint8_t* d_use, AtWork* wk,
                hipStream_t s) {
  const int ldt = at_ldt(T);
  const int64_t n_pad = at_pad4(n_ind);
  const size_t yc_bytes = (((size_t)n_pad * ldt * sizeof(double)) + 255) & ~(size_t)255;
  int rc;
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_p64, yc_bytes + (size_t)n_pad + 256)) != GNX_OK) return rc;
  wk->Yc = (double*)ctx->ws_p64.p;
  wk->part = (uint8_t*)ctx->ws_p64.p + yc_bytes;
  if ((rc = gnx_sum_bad_counter(ctx, 1, &wk->d_bad, s)) != GNX_OK) return rc;
  if (n_pad > 0) {
    hipLaunchKernelGGL(k_ancestry_assoc_traits_prep, dim3((unsigned)((n_pad + 255) / 256)), dim3(256), 0, s, d_Y, ldy, (int)T, d_Z, d_use, n_ind, n_pad,
                       (int)K, ldt, wk->Yc, wk->part);
    HIPCHK(ctx, hipGetLastError());
  }
  return GNX_OK;
}

// host outputs of one call: the three blocks in ws_b64
struct AtOut {
  size_t sy, wy, wyy;
  double *d_sy, *d_wy, *d_wyy;
};

int traits_out(gnx_ctx* ctx, int32_t A, int32_t K, int32_t T, int64_t M, int64_t W, int64_t c0, int64_t c1, AtOut* o) {
  const size_t ldt = (size_t)at_ldt(T), nc = (size_t)(c1 - c0), nw = (size_t)(as_win(c1 - 1, M, W) - as_win(c0, M, W) + 1);
  const auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  o->sy = nc * A * ldt * 8, o->wy = nw * (size_t)(K + A - 1) * ldt * 8, o->wyy = nw * ldt * 8;
  const int rc = gnx_ws_reserve(ctx, ctx->ws_b64, up(o->sy) + up(o->wy) + o->wyy + 64);
  if (rc != GNX_OK) return rc;
  char* base = (char*)ctx->ws_b64.p;
  o->d_sy = (double*)base, o->d_wy = (double*)(base + up(o->sy)), o->d_wyy = (double*)(base + up(o->sy) + up(o->wy));
  return GNX_OK;
}

// the three blocks -> the host; synchronises the stream
int traits_copy_out(gnx_ctx* ctx, const AtOut& o, double* snp_y, double* win_y, double* win_yy, hipStream_t s) {
  HIPCHK(ctx, hipMemcpyAsync(snp_y, o.d_sy, o.sy, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipMemcpyAsync(win_y, o.d_wy, o.wy, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipMemcpyAsync(win_yy, o.d_wyy, o.wyy, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  return GNX_OK;
}

}  // namespace

extern "C" int gnx_ancestry_assoc_traits_dev(gnx_ctx* ctx, const void* d_rows, int row_kind, int64_t ld_rows, const int32_t* d_labels, int64_t ld_labels,
                                             int64_t N, int64_t C, int64_t M, int64_t W, int32_t A, const double* d_Y, int64_t ldy, int32_t T,
                                             const double* d_Z, int32_t K, const uint8_t* d_use, int32_t min_ac, int64_t c0, int64_t c1,
                                             double* d_snp_y, double* d_win_y, double* d_win_yy, int64_t* n_bad) {
  if (!ctx) return GNX_EINVAL;
  int rc = traits_check(ctx, false, d_rows, row_kind, ld_rows, d_labels, ld_labels, N, C, M, W, A, d_Y, ldy, T, d_Z, K, min_ac, c0, c1, d_snp_y, d_win_y,
                        d_win_yy);
  if (rc != GNX_OK) return rc;
  GNX_BIND_DEVICE(ctx);
  hipStream_t s = ctx->stream;
  AtWork wk;
  if ((rc = traits_work(ctx, N / 2, K, T, d_Y, ldy, d_Z, d_use, &wk, s)) != GNX_OK) return rc;
  HIPCHK(ctx, traits_launch(d_rows, row_kind, ld_rows, d_labels, ld_labels, N / 2, M, W, A, K, T, c0, c1, d_Z, wk.Yc, wk.part, 0, d_snp_y, d_win_y,
                            d_win_yy, wk.d_bad, s));
  return gnx_sum_read_verdict(ctx, AT_WHO, wk.d_bad, A, AT_TAIL, n_bad, s);
}

extern "C" int gnx_ancestry_assoc_traits(gnx_ctx* ctx, const int8_t* X, int64_t ld_rows, const int32_t* labels, int64_t ld_labels, int64_t N, int64_t C,
                                         int64_t M, int64_t W, int32_t A, const double* Y, int64_t ldy, int32_t T, const double* Z, int32_t K,
                                         const uint8_t* use, int32_t min_ac, int64_t c0, int64_t c1, double* snp_y, double* win_y, double* win_yy,
                                         int64_t* n_bad) {
  if (!ctx) return GNX_EINVAL;
  int rc = traits_check(ctx, false, X, GNX_ROWS_INT8, ld_rows, labels, ld_labels, N, C, M, W, A, Y, ldy, T, Z, K, min_ac, c0, c1, snp_y, win_y, win_yy);
  if (rc != GNX_OK) return rc;
  GNX_BIND_DEVICE(ctx);
  hipStream_t s = ctx->stream;
  // inputs: rows -> ws_xu, labels -> ws_lab, Y | Z | use -> ws_scale; outputs: the three blocks in ws_b64
  gnx_sum_traits ph;
  AtOut o;
  if ((rc = gnx_sum_stage_rows_labels(ctx, X, GNX_ROWS_INT8, ld_rows, labels, ld_labels, N, C, W, s)) != GNX_OK) return rc;
  if ((rc = gnx_sum_stage_traits(ctx, Y, ldy, T, Z, K, use, N / 2, &ph, s)) != GNX_OK) return rc;
  if ((rc = traits_out(ctx, A, K, T, M, W, c0, c1, &o)) != GNX_OK) return rc;
  rc = gnx_ancestry_assoc_traits_dev(ctx, ctx->ws_xu.p, GNX_ROWS_INT8, ld_rows, (const int32_t*)ctx->ws_lab.p, ld_labels, N, C, M, W, A, ph.d_Y, T, T,
                                     ph.d_Z, K, ph.d_use, min_ac, c0, c1, o.d_sy, o.d_wy, o.d_wyy, n_bad);
  if (rc != GNX_OK && rc != GNX_EINVAL) return rc;
  // (GNX_EINVAL after the launch = labels out of range: the other values stand and are handed over)
  const std::string msg = ctx->err;
  const int rc2 = traits_copy_out(ctx, o, snp_y, win_y, win_yy, s);
  if (rc2 != GNX_OK) return rc2;
  ctx->err = msg;
  return rc;
}

// The file path's form: the packed rows of gnx_infer_gt2's batches (gnx_summary_host.h), reduced against the caller's labels batch by
// batch.  A batch holds whole groups of 4 individuals (8 haplotypes) in ascending order, whatever GNX_HOST_BATCH says, and goes on from
// the accumulators of the batches before it: every MFMA sees the four individuals a single launch gives it, so the blocks equal the
// matrix path's bit for bit at any batch size.
extern "C" int gnx_ancestry_assoc_traits_gt2(gnx_model* m, const uint8_t* G, int64_t V, int64_t ldg, int64_t N, const int32_t* src,
                                             const int32_t* labels, const double* Y, int64_t ldy, int32_t T, const double* Z, int32_t K,
                                             const uint8_t* use, int32_t min_ac, int64_t c0, int64_t c1, double* snp_y, double* win_y, double* win_yy,
                                             int64_t* n_bad) {
  if (!m) return GNX_EINVAL;
  gnx_ctx* ctx = m->ctx;
  const int64_t C = m->info.C, M = m->info.M, W = m->info.W;
  const int32_t A = m->info.A;
  int rc = gnx_sum_gt2_args(ctx, "ancestry_assoc_traits_gt2", G, V, ldg, N, src);
  if (rc != GNX_OK) return rc;
  if ((rc = traits_check(ctx, true, nullptr, GNX_ROWS_PACKED2, (C + 3) / 4, labels, W, N, C, M, W, A, Y, ldy, T, Z, K, min_ac, c0, c1, snp_y, win_y,
                         win_yy)) != GNX_OK)
    return rc;
  if ((rc = gnx_sum_check_src(ctx, "ancestry_assoc_traits_gt2", src, C, V)) != GNX_OK) return rc;
  GNX_BIND_DEVICE(ctx);
  hipStream_t s = ctx->stream;
  gnx_sum_gt2 st;
  gnx_sum_traits ph;
  AtWork wk;
  AtOut o;
  if ((rc = gnx_sum_gt2_stage(ctx, G, V, ldg, N, src, labels, C, W, true, &st, s)) != GNX_OK) return rc;
  const int64_t nb8 = std::max<int64_t>(8, st.nb / 8 * 8);   // haplotypes per batch here: whole groups of 4 individuals
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_xu, (size_t)nb8 * st.ldp + 256)) != GNX_OK) return rc;
  if ((rc = gnx_sum_stage_traits(ctx, Y, ldy, T, Z, K, use, N / 2, &ph, s)) != GNX_OK) return rc;
  if ((rc = traits_work(ctx, N / 2, K, T, ph.d_Y, T, ph.d_Z, ph.d_use, &wk, s)) != GNX_OK) return rc;
  if ((rc = traits_out(ctx, A, K, T, M, W, c0, c1, &o)) != GNX_OK) return rc;
  const int ldt = at_ldt(T);
  if (N == 0)   // no individuals: the blocks of nobody
    HIPCHK(ctx, traits_launch(ctx->ws_xu.p, GNX_ROWS_PACKED2, st.ldp, st.d_lab, W, 0, M, W, A, K, T, c0, c1, ph.d_Z, wk.Yc, wk.part, 0, o.d_sy, o.d_wy,
                              o.d_wyy, wk.d_bad, s));
  for (int64_t n0 = 0; n0 < N; n0 += nb8) {
    const int64_t n = std::min(nb8, N - n0);
    HIPCHK(ctx, gnx_sum_gt2_batch(st, n0, n, C, ctx->ws_xu.p, s));
    HIPCHK(ctx, traits_launch(ctx->ws_xu.p, GNX_ROWS_PACKED2, st.ldp, st.d_lab + n0 * W, W, n / 2, M, W, A, K, T, c0, c1, ph.d_Z + (n0 / 2) * K,
                              wk.Yc + (n0 / 2) * ldt, wk.part + n0 / 2, n0 > 0, o.d_sy, o.d_wy, o.d_wyy, wk.d_bad, s));
  }
  unsigned long long h_bad = 0;
  HIPCHK(ctx, hipMemcpyAsync(&h_bad, wk.d_bad, sizeof h_bad, hipMemcpyDeviceToHost, s));
  if ((rc = traits_copy_out(ctx, o, snp_y, win_y, win_yy, s)) != GNX_OK) return rc;
  return gnx_sum_label_verdict(ctx, "ancestry_assoc_traits_gt2", h_bad, A, AT_TAIL, n_bad);
}
