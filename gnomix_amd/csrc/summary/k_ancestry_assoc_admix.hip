// summary/k_ancestry_assoc_admix.hip — admixture mapping: the sufficient statistics of the regression of T traits on the LOCAL ANCESTRY
// itself, window by window, from the labels alone (no genotypes) on the float64 matrix cores (include/gnomix_hip.h states the contract;
// DESIGN.md 4.24).  The finish (per-ancestry and joint tests, max-T permutations) is the host's: gnomix_amd/admixmap.py.
//
// labels (N, W) int32 (row stride ldl), rows 2 i and 2 i + 1 are individual i; Y (N / 2, T) float64 (row stride ldy); Z (N / 2, K).
// Individual i takes part at window k when use[i] != 0, Z[i, :] is finite, EVERY entry of Y[i, :] is finite and both labels at k lie in
// [0, A) (labels are only compared, never used as an index).  h_a[i, k] in {0, 1, 2}: how many of i's two labels at k equal a.
// ldt = T rounded up to a multiple of 16; n_pad = N / 2 rounded up to a multiple of 4.
//
// k_ancestry_assoc_admix_prep: 16 lanes per individual i < n_pad (Y is read and Yc written in 128-byte segments): part[i] (takes part
//   as far as use, Z and Y say; 0 for i >= N / 2) and the cleaned copy Yc (n_pad, ldt): Yc[i, t] = Y[i, t] where part[i] and t < T, else +0.0.  No NaN or infinity reaches the matrix pipe.
// Both product kernels: a workgroup of 4 waves owns a tile of 16 adjacent windows of [w0, w1) and walks ALL individuals in ascending
//   chunks of AM_CH = 32.  Per chunk it stages in LDS, once for its 16 windows:
//     code[i][j]   the two labels of individual i at window j of the tile, one 64-byte segment per haplotype row (16 lanes read 16
//                  adjacent labels), as la | lb << 8, or AM_OUT where the individual takes no part at that window;
//     z[i][k]      the covariates.
//   Windows past w1 of the last tile repeat window w1 - 1 and individuals past the last one are AM_OUT: no load leaves its array, nothing
//   branches per lane, and such windows are never stored.  A column p of U = [Z, h_0 .. h_{A-1}, 1] of individual i at window j is
//     p < K: z[i][p];  p < K + A: (la == p - K) + (lb == p - K);  p == K + A: 1;   all of them 0 where code[i][j] == AM_OUT (a select:
//     a non-participant's Z may be NaN) and for p > K + A.
//   Wave v takes the windows v, v + 4, v + 8, v + 12 of the tile.  v_mfma_f64_16x16x4_f64 with K = 4 consecutive individuals:
//     A operand of lane l: U[i0 + (l >> 4)][16 mt + (l & 15)];  B operand: column 16 nt + (l & 15) of the same 4 individuals;
//     C / D: column = l & 15, row = (l >> 4) + 4 reg.
// k_ancestry_assoc_admix_main<MT, NT>: B = Yc, the chunk's segments staged in LDS once and shared by the 16 windows; a workgroup carries
//   NT trait tiles (grid.y walks the groups) and all MT = ceil((K + A) / 16) row tiles, MT * NT <= 4: 4 windows x MT x NT accumulators of
//   8 VGPRs per wave.  -> win_y.  diag(Y^T Y): wave v < NT issues one more MFMA per group with M = the 16 WINDOWS of the tile (A operand:
//   takes part at window l & 15, 1.0 or 0.0) and B = Yc^2 (the square rounded once) of trait tile v.  -> win_yy.
// k_ancestry_assoc_admix_gram: B = U itself, one pair (mt <= nt) of tiles of the (K + A + 1)^2 Gram matrix per workgroup (grid.y walks
//   the pairs).  Z^T Z (upper triangle) and Z^T H leave as float64 -> win_g; H^T H, H^T 1 = hs and 1^T 1 = n are sums of integers <= 4,
//   exact in float64 below 2^53, and leave as int32 -> win_i.  Block row 0 also counts the labels outside [0, A) among ALL rows.
//
// SUMMATION ORDER.  Every float sum starts at +0.0 and runs over the individuals in ascending groups of 4 (i = 4 g .. 4 g + 3), one MFMA
// per group; non-participants enter as zeros; the order of the four terms inside one instruction is the hardware's.  The same for every
// window, tile and template: a value is a function of N and the data alone, not of the grid, NT, [w0, w1), ldl or ldy.  Every output
// has one owning wave and leaves with a plain vector store: no atomics on an output, nothing to zero first.  No per-thread array is
// indexed at run time; no scratch.
#include "gnx_summary_host.h"

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int AM_THREADS = 256;
constexpr int AM_CH = 32;            // individuals per chunk: 8 groups of 4
constexpr int AM_WT = 16;            // windows per workgroup
constexpr uint32_t AM_OUT = 0xFFFFu; // the code of an individual that takes no part at a window
constexpr int AM_MAX_A = GNX_ALLELE_MAX_A;
constexpr int AM_MAX_K = GNX_ASSOC_MAX_K;
constexpr int AM_MAX_T = GNX_ASSOC_MAX_T;

inline int am_ldt(int T) { return (T + 15) / 16 * 16; }
inline int64_t am_pad4(int64_t n) { return (n + 3) / 4 * 4; }

// 16 lanes per individual, 16 individuals per workgroup: a lane reads the columns t = l, l + 16, .. of its row (16 lanes = one 128-byte
// segment), the 16 verdicts meet in a ballot, and the row of Yc is written the same way
__global__ __launch_bounds__(256) void k_ancestry_assoc_admix_prep(const double* __restrict__ Y, int64_t ldy, int T, const double* __restrict__ Z,
                                                                   const uint8_t* __restrict__ use, int64_t n_ind, int64_t n_pad, int K, int ldt,
                                                                   double* __restrict__ Yc, uint8_t* __restrict__ part) {
  const int l16 = threadIdx.x & 15;
  const int64_t i = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  bool ok = i < n_ind && (use == nullptr || use[i] != 0);
  if (ok) {
    for (int k = l16; k < K; k += 16) ok = ok && isfinite(Z[i * K + k]);
    for (int t = l16; t < T; t += 16) ok = ok && isfinite(Y[i * ldy + t]);
  }
  const unsigned long long m = __ballot(ok);   // every lane of the wave is here: nothing returned above
  const bool row_ok = ((m >> (threadIdx.x & 48)) & 0xFFFFull) == 0xFFFFull;
  if (i >= n_pad) return;
  double* yc = Yc + i * ldt;
  for (int t = l16; t < ldt; t += 16) yc[t] = (row_ok && t < T) ? Y[i * ldy + t] : 0.0;
  if (l16 == 0) part[i] = row_ok ? 1 : 0;
}

// the chunk [ci0, ci0 + AM_CH): the codes of the tile's 16 windows and the covariates -> LDS; returns this thread's count of labels outside
// [0, A) among the rows and windows that exist (each (row, window) is looked at by exactly one thread)
__device__ __forceinline__ unsigned am_stage(const int32_t* __restrict__ lab, int64_t ldl, int64_t n_ind, int A, int K, int64_t wt0, int64_t w1,
                                             const double* __restrict__ Z, const uint8_t* __restrict__ part, int64_t ci0,
                                             uint16_t (*code)[AM_WT], double (*z)[AM_MAX_K]) {
  const int tid = threadIdx.x, j = tid & 15, r = tid >> 4;
  const bool wlive = wt0 + j < w1;
  const int64_t w = wlive ? wt0 + j : w1 - 1;
  unsigned nbad = 0;
#pragma unroll
  for (int h = 0; h < AM_CH / 16; ++h) {
    const int64_t i = ci0 + r + 16 * h;
    const bool live = i < n_ind;
    const int64_t ii = live ? i : n_ind - 1;   // (n_ind >= 1 here: no chunk is walked otherwise)
    const int32_t la = lab[(2 * ii) * ldl + w], lb = lab[(2 * ii + 1) * ldl + w];
    const bool oka = la >= 0 && la < A, okb = lb >= 0 && lb < A;
    if (live && wlive) nbad += (oka ? 0u : 1u) + (okb ? 0u : 1u);
    const bool takes = live && oka && okb && part[ii] != 0;
    code[r + 16 * h][j] = (uint16_t)(takes ? ((uint32_t)la | ((uint32_t)lb << 8)) : AM_OUT);
  }
  for (int e = tid; e < AM_CH * K; e += AM_THREADS) {
    const int64_t g = ci0 * K + e;   // Z is contiguous: the chunk's covariates are one run
    z[e / K][e % K] = g < n_ind * K ? Z[g] : 0.0;
  }
  return nbad;
}

// column p of U of one individual: c its code at the window, zrow its covariates in LDS
__device__ __forceinline__ double am_u(uint32_t c, const double* zrow, int p, int K, int A) {
  const bool takes = c != AM_OUT;
  const int a = p - K;
  const double zv = zrow[p < K ? p : K - 1];
  const double hv = (double)(((int)(c & 0xFFu) == a ? 1 : 0) + ((int)(c >> 8) == a ? 1 : 0));   // a >= A matches no label (< A <= 32)
  const double v = p < K ? zv : p < K + A ? hv : p == K + A ? 1.0 : 0.0;
  return takes ? v : 0.0;
}

template <int MT, int NT>
__global__ __launch_bounds__(AM_THREADS) void k_ancestry_assoc_admix_main(const int32_t* __restrict__ lab, int64_t ldl, int64_t n_ind, int A, int K,
                                                                          int64_t w0, int64_t w1, const double* __restrict__ Z,
                                                                          const double* __restrict__ Yc, int ldt, const uint8_t* __restrict__ part,
                                                                          double* __restrict__ win_y, double* __restrict__ win_yy) {
  constexpr int LDY = NT * 16 + (NT > 1 ? 16 : 0);   // the rows of a group of 4 fall on different banks
  __shared__ uint16_t code[AM_CH][AM_WT];
  __shared__ double z[AM_CH][AM_MAX_K];
  __shared__ double ys[AM_CH][LDY];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r16 = lane & 15, kq = lane >> 4;
  const int64_t wt0 = w0 + (int64_t)blockIdx.x * AM_WT;
  const int tt0 = (int)blockIdx.y * NT, n_tt = ldt / 16, P = K + A;

  d4 acc[4][MT][NT];
  d4 acc_yy = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int wi = 0; wi < 4; ++wi)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[wi][mt][j] = d4{0.0, 0.0, 0.0, 0.0};

  for (int64_t ci0 = 0; ci0 < n_ind; ci0 += AM_CH) {
    __syncthreads();   // the chunk before has been read
    am_stage(lab, ldl, n_ind, A, K, wt0, w1, Z, part, ci0, code, z);
    for (int e = tid; e < AM_CH * NT * 16; e += AM_THREADS) {
      const int row = e / (NT * 16), col = e % (NT * 16), tt = tt0 + col / 16;
      const int64_t i = ci0 + row;
      ys[row][col] = (i < n_ind && tt < n_tt) ? Yc[i * ldt + tt * 16 + (col & 15)] : 0.0;
    }
    __syncthreads();
    const int n_g = (int)((n_ind - ci0 < AM_CH ? n_ind - ci0 : AM_CH) + 3) / 4;
    for (int g = 0; g < n_g; ++g) {
      const int il = 4 * g + kq;
      double b[NT];
#pragma unroll
      for (int j = 0; j < NT; ++j) b[j] = ys[il][j * 16 + r16];
#pragma unroll
      for (int wi = 0; wi < 4; ++wi) {
        const uint32_t c = code[il][wv + 4 * wi];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const double a = am_u(c, z[il], mt * 16 + r16, K, A);
#pragma unroll
          for (int j = 0; j < NT; ++j)
            if (tt0 + j < n_tt) acc[wi][mt][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[j], acc[wi][mt][j], 0, 0, 0);
        }
      }
      if (wv < NT && tt0 + wv < n_tt) {   // diag(Y^T Y) of trait tile wv: M = the 16 windows
        const double yv = ys[il][wv * 16 + r16];
        const double t1 = code[il][r16] != AM_OUT ? 1.0 : 0.0;
        acc_yy = __builtin_amdgcn_mfma_f64_16x16x4f64(t1, yv * yv, acc_yy, 0, 0, 0);
      }
    }
  }

#pragma unroll
  for (int wi = 0; wi < 4; ++wi) {
    const int64_t wk = wt0 + wv + 4 * wi;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int p = mt * 16 + kq + 4 * r;
          if (wk < w1 && p < P && tt0 + j < n_tt) win_y[((wk - w0) * P + p) * ldt + (tt0 + j) * 16 + r16] = acc[wi][mt][j][r];
        }
  }
  if (wv < NT && tt0 + wv < n_tt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t wk = wt0 + kq + 4 * r;
      if (wk < w1) win_yy[(wk - w0) * ldt + (tt0 + wv) * 16 + r16] = acc_yy[r];
    }
  }
}

__global__ __launch_bounds__(AM_THREADS) void k_ancestry_assoc_admix_gram(const int32_t* __restrict__ lab, int64_t ldl, int64_t n_ind, int A, int K,
                                                                          int64_t w0, int64_t w1, const double* __restrict__ Z,
                                                                          const uint8_t* __restrict__ part, int32_t* __restrict__ win_i,
                                                                          double* __restrict__ win_g, unsigned long long* __restrict__ bad) {
  __shared__ uint16_t code[AM_CH][AM_WT];
  __shared__ double z[AM_CH][AM_MAX_K];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r16 = lane & 15, kq = lane >> 4;
  const int64_t wt0 = w0 + (int64_t)blockIdx.x * AM_WT;
  const int Q = K + A + 1, n_q = (Q + 15) / 16;
  // the pair (mt <= nt) of this workgroup: blockIdx.y counts them row by row
  int mt = 0, nt = (int)blockIdx.y;
  while (nt >= n_q - mt) {
    nt -= n_q - mt;
    ++mt;
  }
  nt += mt;

  d4 acc[4];
#pragma unroll
  for (int wi = 0; wi < 4; ++wi) acc[wi] = d4{0.0, 0.0, 0.0, 0.0};
  unsigned nbad = 0;

  for (int64_t ci0 = 0; ci0 < n_ind; ci0 += AM_CH) {
    __syncthreads();
    nbad += am_stage(lab, ldl, n_ind, A, K, wt0, w1, Z, part, ci0, code, z);
    __syncthreads();
    const int n_g = (int)((n_ind - ci0 < AM_CH ? n_ind - ci0 : AM_CH) + 3) / 4;
    for (int g = 0; g < n_g; ++g) {
      const int il = 4 * g + kq;
#pragma unroll
      for (int wi = 0; wi < 4; ++wi) {
        const uint32_t c = code[il][wv + 4 * wi];
        const double a = am_u(c, z[il], mt * 16 + r16, K, A), b = am_u(c, z[il], nt * 16 + r16, K, A);
        acc[wi] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[wi], 0, 0, 0);
      }
    }
  }
  if (blockIdx.y == 0 && nbad) atomicAdd(bad, (unsigned long long)nbad);

  const int NI = 1 + A + A * (A + 1) / 2, NG = K * (K + 1) / 2 + K * A;
  const int q = nt * 16 + r16;
#pragma unroll
  for (int wi = 0; wi < 4; ++wi) {
    const int64_t wk = wt0 + wv + 4 * wi;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int p = mt * 16 + kq + 4 * r;
      if (wk >= w1 || p > q || q >= Q) continue;
      const double v = acc[wi][r];
      int32_t* wi32 = win_i + (wk - w0) * NI;
      double* wg = win_g + (wk - w0) * NG;
      if (p < K) {
        if (q < K) wg[p * K - p * (p - 1) / 2 + (q - p)] = v;
        else if (q < K + A) wg[K * (K + 1) / 2 + p * A + (q - K)] = v;
      } else if (p < K + A) {
        const int a = p - K, b = q - K;
        if (q < K + A) wi32[1 + A + a * A - a * (a - 1) / 2 + (b - a)] = (int32_t)v;
        else wi32[1 + a] = (int32_t)v;
      } else {
        wi32[0] = (int32_t)v;
      }
    }
  }
}

const char* const AM_TAIL = "an individual with such a label takes no part at that window";
const char* const AM_WHO = "ancestry_admixmap";

// every refusal before the launch; GNX_OK or the code
int admix_check(gnx_ctx* ctx, const void* labels, int64_t ld_labels, int64_t N, int64_t W, int32_t A, const void* Y, int64_t ldy, int32_t T, const void* Z,
                int32_t K, int64_t w0, int64_t w1, const void* win_i, const void* win_g, const void* win_y, const void* win_yy) {
  const std::string w(AM_WHO);
  if (!ctx->usable) return gnx_fail(ctx, GNX_ESTATE, "context has no device (gnx_init failed)");
  if (N < 0 || W < 1 || A < 1) return gnx_fail(ctx, GNX_EINVAL, w + ": need N >= 0, W >= 1 and A >= 1");
  if (ld_labels < W) return gnx_fail(ctx, GNX_EINVAL, w + ": the labels' row stride is smaller than W");
  if (K < 1) return gnx_fail(ctx, GNX_EINVAL, w + ": need K >= 1 covariates (the caller supplies the intercept column)");
  if (T < 1 || ldy < T) return gnx_fail(ctx, GNX_EINVAL, w + ": need T >= 1 traits and a row stride of Y of at least T");
  if (w0 < 0 || w1 > W || w0 >= w1) return gnx_fail(ctx, GNX_EINVAL, w + ": need 0 <= w0 < w1 <= W");
  if (!labels || !Y || !Z || !win_i || !win_g || !win_y || !win_yy)
    return gnx_fail(ctx, GNX_EINVAL, w + ": a null pointer (only use and n_bad may be NULL)");
  if (A > AM_MAX_A) return gnx_fail(ctx, GNX_EUNSUPPORTED, w + ": A = " + std::to_string(A) + " ancestries, at most " + std::to_string(AM_MAX_A));
  if (K > AM_MAX_K) return gnx_fail(ctx, GNX_EUNSUPPORTED, w + ": K = " + std::to_string(K) + " covariates, at most " + std::to_string(AM_MAX_K));
  if (T > AM_MAX_T) return gnx_fail(ctx, GNX_EUNSUPPORTED, w + ": T = " + std::to_string(T) + " traits, at most " + std::to_string(AM_MAX_T));
  if (N > ((int64_t)1 << 28)) return gnx_fail(ctx, GNX_EUNSUPPORTED, w + ": N must not exceed 2^28 (the integer blocks are int32)");
  if (N % 2) return gnx_fail(ctx, GNX_EUNSUPPORTED, w + ": N must be even (an individual has two haplotype rows)");
  return GNX_OK;
}

// false: no template carries MT x nt (the caller's choice of nt keeps MT * nt <= 4; a launch that would be skipped is an error, never silence)
template <int MT>
bool admix_main_launch(int nt, dim3 grid, hipStream_t s, const int32_t* lab, int64_t ldl, int64_t n_ind, int A, int K, int64_t w0, int64_t w1,
                       const double* Z, const double* Yc, int ldt, const uint8_t* part, double* win_y, double* win_yy) {
  if (nt == 1)
    hipLaunchKernelGGL((k_ancestry_assoc_admix_main<MT, 1>), grid, dim3(AM_THREADS), 0, s, lab, ldl, n_ind, A, K, w0, w1, Z, Yc, ldt, part, win_y, win_yy);
  else if (nt == 2) {
    if constexpr (MT * 2 <= 4)
      hipLaunchKernelGGL((k_ancestry_assoc_admix_main<MT, 2>), grid, dim3(AM_THREADS), 0, s, lab, ldl, n_ind, A, K, w0, w1, Z, Yc, ldt, part, win_y, win_yy);
    else
      return false;
  } else if (nt == 4) {
    if constexpr (MT * 4 <= 4)
      hipLaunchKernelGGL((k_ancestry_assoc_admix_main<MT, 4>), grid, dim3(AM_THREADS), 0, s, lab, ldl, n_ind, A, K, w0, w1, Z, Yc, ldt, part, win_y, win_yy);
    else
      return false;
  } else {
    return false;
  }
  return true;
}

}  // namespace

extern "C" int gnx_ancestry_admixmap_dev(gnx_ctx* ctx, const int32_t* d_labels, int64_t ld_labels, int64_t N, int64_t W, int32_t A, const double* d_Y,
                                         int64_t ldy, int32_t T, const double* d_Z, int32_t K, const uint8_t* d_use, int64_t w0, int64_t w1,
                                         int32_t* d_win_i, double* d_win_g, double* d_win_y, double* d_win_yy, int64_t* n_bad) {
  if (!ctx) return GNX_EINVAL;
  int rc = admix_check(ctx, d_labels, ld_labels, N, W, A, d_Y, ldy, T, d_Z, K, w0, w1, d_win_i, d_win_g, d_win_y, d_win_yy);
  if (rc != GNX_OK) return rc;
  GNX_BIND_DEVICE(ctx);
  hipStream_t s = ctx->stream;
  const int64_t n_ind = N / 2, n_pad = am_pad4(n_ind);
  const int ldt = am_ldt(T), n_tt = ldt / 16;
  // the workspace: Yc | part in ws_p64, the zeroed counter of labels out of range in ws_misc
  const size_t yc_bytes = (((size_t)n_pad * ldt * sizeof(double)) + 255) & ~(size_t)255;
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_p64, yc_bytes + (size_t)n_pad + 256)) != GNX_OK) return rc;
  double* Yc = (double*)ctx->ws_p64.p;
  uint8_t* part = (uint8_t*)ctx->ws_p64.p + yc_bytes;
  unsigned long long* d_bad = nullptr;
  if ((rc = gnx_sum_bad_counter(ctx, 1, &d_bad, s)) != GNX_OK) return rc;
  if (n_pad > 0) {
    hipLaunchKernelGGL(k_ancestry_assoc_admix_prep, dim3((unsigned)((n_pad + 15) / 16)), dim3(256), 0, s, d_Y, ldy, (int)T, d_Z, d_use, n_ind, n_pad,
                       (int)K, ldt, Yc, part);
    HIPCHK(ctx, hipGetLastError());
  }
  const unsigned n_wt = (unsigned)((w1 - w0 + AM_WT - 1) / AM_WT);   // <= W / 16 + 1
  const int n_q = (K + A + 1 + 15) / 16;                              // <= 4: at most 10 pairs
  hipLaunchKernelGGL(k_ancestry_assoc_admix_gram, dim3(n_wt, (unsigned)(n_q * (n_q + 1) / 2)), dim3(AM_THREADS), 0, s, d_labels, ld_labels, n_ind, (int)A,
                     (int)K, w0, w1, d_Z, part, d_win_i, d_win_g, d_bad);
  HIPCHK(ctx, hipGetLastError());
  // MT row tiles of [Z, H] and NT trait tiles per workgroup, MT * NT <= 4 (n_tt = 3 at MT = 1: two groups of 2)
  const int mt = (K + A + 15) / 16, cap = mt == 1 ? 4 : mt == 2 ? 2 : 1;
  const int nt = (n_tt >= 4 && cap >= 4) ? 4 : (n_tt >= 2 && cap >= 2) ? 2 : 1;
  const dim3 grid(n_wt, (unsigned)((n_tt + nt - 1) / nt));            // grid.y <= 4096
  const bool launched = mt == 1   ? admix_main_launch<1>(nt, grid, s, d_labels, ld_labels, n_ind, A, K, w0, w1, d_Z, Yc, ldt, part, d_win_y, d_win_yy)
                        : mt == 2 ? admix_main_launch<2>(nt, grid, s, d_labels, ld_labels, n_ind, A, K, w0, w1, d_Z, Yc, ldt, part, d_win_y, d_win_yy)
                                  : admix_main_launch<3>(nt, grid, s, d_labels, ld_labels, n_ind, A, K, w0, w1, d_Z, Yc, ldt, part, d_win_y, d_win_yy);
  if (!launched) return gnx_fail(ctx, GNX_ESTATE, std::string(AM_WHO) + ": no kernel for this tiling");
  HIPCHK(ctx, hipGetLastError());
  return gnx_sum_read_verdict(ctx, AM_WHO, d_bad, A, AM_TAIL, n_bad, s);
}

extern "C" int gnx_ancestry_admixmap(gnx_ctx* ctx, const int32_t* labels, int64_t ld_labels, int64_t N, int64_t W, int32_t A, const double* Y, int64_t ldy,
                                     int32_t T, const double* Z, int32_t K, const uint8_t* use, int64_t w0, int64_t w1, int32_t* win_i, double* win_g,
                                     double* win_y, double* win_yy, int64_t* n_bad) {
  if (!ctx) return GNX_EINVAL;
  int rc = admix_check(ctx, labels, ld_labels, N, W, A, Y, ldy, T, Z, K, w0, w1, win_i, win_g, win_y, win_yy);
  if (rc != GNX_OK) return rc;
  GNX_BIND_DEVICE(ctx);
  hipStream_t s = ctx->stream;
  // inputs: labels -> ws_lab, Y | Z | use -> ws_scale (Y compact); outputs: the four blocks in ws_b64
  const size_t bl = N > 0 ? ((size_t)(N - 1) * (size_t)ld_labels + (size_t)W) * sizeof(int32_t) : 0;   // the last row ends after its W labels
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_lab, bl + 64)) != GNX_OK) return rc;
  if (bl) HIPCHK(ctx, hipMemcpyAsync(ctx->ws_lab.p, labels, bl, hipMemcpyHostToDevice, s));
  gnx_sum_traits ph;
  if ((rc = gnx_sum_stage_traits(ctx, Y, ldy, T, Z, K, use, N / 2, &ph, s)) != GNX_OK) return rc;
  const size_t nw = (size_t)(w1 - w0), ldt = (size_t)am_ldt(T);
  const auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t bi = nw * (size_t)(1 + A + A * (A + 1) / 2) * 4, bg = nw * (size_t)(K * (K + 1) / 2 + K * A) * 8, by = nw * (size_t)(K + A) * ldt * 8,
               byy = nw * ldt * 8;
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_b64, up(bi) + up(bg) + up(by) + byy + 64)) != GNX_OK) return rc;
  char* base = (char*)ctx->ws_b64.p;
  int32_t* d_i = (int32_t*)base;
  double *d_g = (double*)(base + up(bi)), *d_y = (double*)(base + up(bi) + up(bg)), *d_yy = (double*)(base + up(bi) + up(bg) + up(by));
  rc = gnx_ancestry_admixmap_dev(ctx, (const int32_t*)ctx->ws_lab.p, ld_labels, N, W, A, ph.d_Y, T, T, ph.d_Z, K, ph.d_use, w0, w1, d_i, d_g, d_y, d_yy,
                                 n_bad);
  if (rc != GNX_OK && rc != GNX_EINVAL) return rc;
  // (GNX_EINVAL after the launch = labels out of range: the other values stand and are handed over)
  const std::string msg = ctx->err;
  HIPCHK(ctx, hipMemcpyAsync(win_i, d_i, bi, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipMemcpyAsync(win_g, d_g, bg, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipMemcpyAsync(win_y, d_y, by, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipMemcpyAsync(win_yy, d_yy, byy, hipMemcpyDeviceToHost, s));
  HIPCHK(ctx, hipStreamSynchronize(s));
  ctx->err = msg;
  return rc;
}
