// k_train_lda.hip — the integer half of fitting the LDA base (LDABase) on gfx950: per window the exact Gram matrix of the fit rows,
// the class sums and the class counts, from ONE product on the int8 matrix cores.
//
// Replaces the data pass of LDABase.train (reference src/Base/models.py -> sklearn LinearDiscriminantAnalysis() per window,
// through Base.train_vectorized, src/Base/base.py:104-127).  Everything scikit-learn's _solve_svd consumes is a function of
//   G[w]   = Xw^T Xw                          (width, width) int32
//   S[w,k] = sum of the rows with y[n, w] = k  (A, width)     int32
//   n[w,k] = number of those rows              (A,)           int32
// (gnomix_amd.train.lda_finish turns them into coef_ / intercept_ in float64 on the host).  Xw is the window's slice of the
// reflect-padded row (gnx_window.h), the SNP codes 0..2 as numbers.
//
// One product.  Z = [Xw | onehot(y[:, w])] is (N, width + A); Z^T Z holds G in its top-left block, S in the rows below it and n on
// the diagonal of the one-hot block.  The kernel computes the 64 x 64 macro-tiles of Z^T Z on or below the diagonal with
// v_mfma_i32_16x16x64_i8 and mirrors G on store.  Every product is an integer in [0, 4] and a sum is at most 4 N, so int32 is exact
// for 4 N < 2^31 (refused beyond).
// Layout:
//  * grid = (macro-tile pairs bi >= bj, windows of the range); a block = 4 waves, wave v owns rows 16 v .. 16 v + 15 of the row
//    macro-tile and all four 16-column tiles of the column macro-tile (four int32x4 accumulators);
//  * the reduction index is the haplotype, and X is contiguous along SNPs: per chunk of 64 haplotypes both macro-tiles' columns are
//    staged TRANSPOSED into LDS, t[column][haplotype], four haplotypes per thread and store; a wave's 64 lanes take 64 consecutive
//    columns, so its byte loads of one row of X are one 64-byte segment.  Rows >= N and columns >= width + A are zeros: N is padded
//    to the MFMA's K and the width to the tile with zeros, which add nothing;
//  * LDS row pitch 80 bytes: the 16-byte operand reads of 16 consecutive columns start 20 banks apart, which covers the 64 banks once
//    (conflict-free); the dword stores of 64 consecutive columns are 4-way (20 c mod 64 takes 16 values).  The stores are a small
//    share of a chunk next to its byte loads;
//  * both operands are 16 aligned bytes of a staged row (A: row = lane & 15 of the wave's row tile, B: column = lane & 15, k-block
//    = lane >> 4), the layout k_knn_argmin uses; C/D: column = lane & 15, row = 4 (lane >> 4) + reg.
// No scratch, no atomics, no runtime-indexed register array, plain vector stores.
#include "../gnx_internal.h"
#include "../gnx_window.h"

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int LG_T = 64;          // macro-tile edge (columns of Z)
constexpr int LG_K = 64;          // haplotypes per chunk = the MFMA's K
constexpr int LG_P = LG_K + 16;   // LDS row pitch, bytes
constexpr int LG_ITEMS = 2 * LG_T * (LG_K / 4) / 256;  // (column, 4 haplotypes) items per thread and chunk
constexpr int32_t LG_ZERO = INT32_MIN;                 // a staged column past width + A

struct LdaGramLaunch {
  const int8_t* X;
  const int32_t* Y;
  int64_t N, ldx, C, M, ctx;
  int32_t W, A, w0, ldw;
  int32_t* G;  // [windows of the range][ldw][ldw]
  int32_t* S;  // [windows of the range][A][ldw]
  int32_t* n;  // [windows of the range][A]
};

__global__ __launch_bounds__(256) void k_lda_gram(LdaGramLaunch L) {
  __shared__ __attribute__((aligned(16))) int8_t tz[2 * LG_T * LG_P];  // the row macro-tile's columns, then the column macro-tile's
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int wl = blockIdx.y, w = L.w0 + wl;
  const int width = (int)gnx_window_width(w, L.W, L.C, L.M, L.ctx);
  const int P = width + L.A;
  // blockIdx.x -> (bi, bj), bi >= bj: bi (bi + 1) / 2 + bj
  int bi = (int)((sqrtf(8.0f * (float)blockIdx.x + 1.0f) - 1.0f) * 0.5f);
  while ((bi + 1) * (bi + 2) / 2 <= (int)blockIdx.x) ++bi;
  while (bi * (bi + 1) / 2 > (int)blockIdx.x) --bi;
  const int bj = (int)blockIdx.x - bi * (bi + 1) / 2;
  if (bi * LG_T >= P) return;  // block-uniform, before any barrier (the last window is wider than the others)

  // what each of this thread's staged columns is: >= 0 the column of X, -1 - k the one-hot column of class k, LG_ZERO zeros
  int32_t src[LG_ITEMS];
#pragma unroll
  for (int it = 0; it < LG_ITEMS; ++it) {
    const int idx = t + 256 * it;
    const int z = ((idx >> 10) ? bj : bi) * LG_T + (idx & 63);
    src[it] = z < width ? (int32_t)gnx_pad_src((int64_t)w * L.M + z, L.C, L.ctx) : z < P ? -1 - (z - width) : LG_ZERO;
  }

  v4i acc[4];
#pragma unroll
  for (int jt = 0; jt < 4; ++jt) acc[jt] = v4i{0, 0, 0, 0};
  const int8_t* ap = tz + (wv * 16 + (lane & 15)) * LG_P + (lane >> 4) * 16;
  const int8_t* bp = tz + (LG_T + (lane & 15)) * LG_P + (lane >> 4) * 16;

  for (int64_t k0 = 0; k0 < L.N; k0 += LG_K) {
#pragma unroll
    for (int it = 0; it < LG_ITEMS; ++it) {
      const int idx = t + 256 * it;
      const int g = (idx & 1023) >> 6;  // haplotypes k0 + 4 g .. + 3
      uint32_t v = 0;
      if (src[it] != LG_ZERO) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t n = k0 + 4 * g + r;
          if (n < L.N) {
            const uint32_t b = src[it] >= 0 ? (uint32_t)(uint8_t)L.X[n * L.ldx + src[it]] : (uint32_t)(L.Y[n * L.W + w] == -1 - src[it]);
            v |= b << (8 * r);
          }
        }
      }
      *reinterpret_cast<uint32_t*>(tz + ((idx >> 10) * LG_T + (idx & 63)) * LG_P + 4 * g) = v;
    }
    __syncthreads();
    const v4i a = *reinterpret_cast<const v4i*>(ap);
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
      const v4i b = *reinterpret_cast<const v4i*>(bp + jt * 16 * LG_P);
      acc[jt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, acc[jt], 0, 0, 0);
    }
    __syncthreads();
  }

  // (zi, zj) of Z^T Z, zi >= zj in every off-diagonal macro-tile; a diagonal macro-tile holds both halves, so an element with
  // zi < width <= zj is left to its mirror image in the same block
  const size_t ldw = (size_t)L.ldw;
  int32_t* Gw = L.G + (size_t)wl * ldw * ldw;
  int32_t* Sw = L.S + (size_t)wl * L.A * ldw;
  int32_t* nw = L.n + (size_t)wl * L.A;
#pragma unroll
  for (int jt = 0; jt < 4; ++jt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int zi = bi * LG_T + wv * 16 + 4 * (lane >> 4) + r;
      const int zj = bj * LG_T + jt * 16 + (lane & 15);
      const int32_t v = acc[jt][r];
      if (zi < width && zj < width) {
        Gw[(size_t)zi * ldw + zj] = v;
        Gw[(size_t)zj * ldw + zi] = v;
      } else if (zi >= width && zi < P && zj < width) {
        Sw[(size_t)(zi - width) * ldw + zj] = v;
      } else if (zi >= width && zi < P && zj == zi) {
        nw[zi - width] = v;
      }
    }
}

int lda_gram_check(gnx_ctx* ctx, const void* X, const void* y, int64_t N, int64_t ldx, int64_t C, int64_t M, int64_t cx, int32_t A,
                   int64_t w0, int64_t w1, const void* G, const void* S, const void* n) {
  if (!ctx->usable) return gnx_fail(ctx, GNX_ESTATE, "context has no device (gnx_init failed)");
  if (!X || !y || !G || !S || !n) return gnx_fail(ctx, GNX_EINVAL, "train_lda_gram: NULL pointer");
  if (A < 2 || A > 32) return gnx_fail(ctx, GNX_EINVAL, "train_lda_gram: A must be in [2, 32]");
  if (M <= 0 || C < M || cx < 0 || cx > C || C > ((int64_t)1 << 30)) return gnx_fail(ctx, GNX_EINVAL, "train_lda_gram: bad C / M / ctx");
  if (N < 1 || ldx < C) return gnx_fail(ctx, GNX_EINVAL, "train_lda_gram: bad N / ldx");
  if (N >= ((int64_t)1 << 29)) return gnx_fail(ctx, GNX_EINVAL, "train_lda_gram: 4 N reaches 2^31 (an int32 sum of code products could overflow)");
  const int64_t W = C / M;
  if (w0 < 0 || w1 <= w0 || w1 > W || w1 - w0 > 65535) return gnx_fail(ctx, GNX_EINVAL, "train_lda_gram: bad window range [w0, w1)");
  if (M + 2 * cx + (C - M * W) + A > 32768) return gnx_fail(ctx, GNX_EINVAL, "train_lda_gram: windows wider than 32768 - A SNPs");
  return GNX_OK;
}

hipError_t lda_gram_run(const int8_t* dX, int64_t N, int64_t ldx, const int32_t* dy, int64_t C, int64_t M, int64_t cx, int32_t A, int64_t w0,
                        int64_t w1, int32_t* G, int32_t* S, int32_t* n, hipStream_t s) {
  const int64_t W = C / M, ldw = M + 2 * cx + (C - M * W), nw = w1 - w0;
  hipError_t e;
  // positions past a window's width (every window but the last is rem narrower than ldw) hold 0
  if ((e = hipMemsetAsync(G, 0, (size_t)nw * ldw * ldw * 4, s)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(S, 0, (size_t)nw * A * ldw * 4, s)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(n, 0, (size_t)nw * A * 4, s)) != hipSuccess) return e;
  LdaGramLaunch L{dX, dy, N, ldx, C, M, cx, (int32_t)W, A, (int32_t)w0, (int32_t)ldw, G, S, n};
  const int T = (int)((ldw + A + LG_T - 1) / LG_T);
  hipLaunchKernelGGL(k_lda_gram, dim3((unsigned)(T * (T + 1) / 2), (unsigned)nw), dim3(256), 0, s, L);
  return hipGetLastError();
}

}  // namespace

extern "C" {

int gnx_train_lda_gram_dev(gnx_ctx* ctx, const int8_t* dX, int64_t N, int64_t ldx, const int32_t* dy, int64_t C, int64_t M, int64_t cx,
                           int32_t A, int64_t w0, int64_t w1, int32_t* d_G, int32_t* d_S, int32_t* d_n) {
  if (!ctx) return GNX_EINVAL;
  int rc = lda_gram_check(ctx, dX, dy, N, ldx, C, M, cx, A, w0, w1, d_G, d_S, d_n);
  if (rc != GNX_OK) return rc;
  GNX_BIND_DEVICE(ctx);
  HIPCHK(ctx, lda_gram_run(dX, N, ldx, dy, C, M, cx, A, w0, w1, d_G, d_S, d_n, ctx->stream));
  return GNX_OK;
}

int gnx_train_lda_gram(gnx_ctx* ctx, const int8_t* X, int64_t N, int64_t ldx, const int32_t* y, int64_t C, int64_t M, int64_t cx, int32_t A,
                       int64_t w0, int64_t w1, int32_t* G, int32_t* S, int32_t* n) {
  if (!ctx) return GNX_EINVAL;
  int rc = lda_gram_check(ctx, X, y, N, ldx, C, M, cx, A, w0, w1, G, S, n);
  if (rc != GNX_OK) return rc;
  const int64_t W = C / M, ldw = M + 2 * cx + (C - M * W), nw = w1 - w0;
  for (int64_t i = 0; i < N; ++i)
    for (int64_t w = w0; w < w1; ++w)
      if (y[i * W + w] < 0 || y[i * W + w] >= A) return gnx_fail(ctx, GNX_EINVAL, "train_lda_gram: label outside [0, A)");
  for (int64_t i = 0; i < N; ++i)
    for (int64_t j = 0; j < C; ++j)
      if ((uint8_t)X[i * ldx + j] > 2) return gnx_fail(ctx, GNX_EINVAL, "train_lda_gram: X holds a code outside {0, 1, 2}");
  GNX_BIND_DEVICE(ctx);
  const size_t gb = (size_t)nw * ldw * ldw * 4, sb = (size_t)nw * A * ldw * 4, cb = (size_t)nw * A * 4;
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_x, (size_t)N * ldx + 64)) != GNX_OK) return rc;
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_lab, (size_t)N * W * 4)) != GNX_OK) return rc;
  if ((rc = gnx_ws_reserve(ctx, ctx->ws_misc, gb + sb + cb)) != GNX_OK) return rc;
  int32_t* dG = (int32_t*)ctx->ws_misc.p;
  int32_t* dS = dG + (size_t)nw * ldw * ldw;
  int32_t* dn = dS + (size_t)nw * A * ldw;
  HIPCHK(ctx, hipMemcpyAsync(ctx->ws_x.p, X, (size_t)(N - 1) * ldx + C, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ctx->ws_lab.p, y, (size_t)N * W * 4, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, lda_gram_run((const int8_t*)ctx->ws_x.p, N, ldx, (const int32_t*)ctx->ws_lab.p, C, M, cx, A, w0, w1, dG, dS, dn, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(G, dG, gb, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(S, dS, sb, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(n, dn, cb, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return GNX_OK;
}

}  // extern "C"
