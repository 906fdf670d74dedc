// k_base_knn.hip — the 1-nearest-neighbour base (KNNBase) on gfx950: an exact integer argmin on the int8 matrix cores.
//
// Replaces KNNBase.predict_proba (reference src/Base/models.py:135-146 through src/Base/base.py:146-180): per window
//   sklearn KNeighborsClassifier(n_neighbors=1).predict_proba(Xw)   (uniform weights, Euclidean metric).
//
// Semantics, complete:
//  * For query haplotype n and window w:  B[n, w, c] = 1 if c == y_fit[i*], else 0, where i* minimises the squared Euclidean
//    distance d2(x_nw, fit_i) over the window's fit rows i = 0 .. n_fit-1.  x_nw is the window's slice of the reflect-padded
//    query (base.py:41-44; width M + 2 ctx, the last window M + 2 ctx + rem).
//  * d2 is an integer: the SNP codes are numbers.  2 = missing is the number 2 (as everywhere in the reference); a query code 3
//    (the largest a 2-bit packed row can hold) is the number 3, as in the RBF base.  Fit rows hold 0..2 (checked at load).  Other
//    int8 query values are outside the contract; nothing overflows or is read out of bounds for them.
//  * TIES GO TO THE LOWEST FIT-ROW INDEX.  This is this library's rule and a documented deviation: scikit-learn's choice among
//    equidistant neighbours depends on the algorithm it resolves to (brute / kd_tree) and is not specified.  Whatever it picks
//    is at the minimum distance, so the outputs agree wherever the minimum-distance rows carry one label.
//  * A class absent from a window's fit labels gets a zero column.  The float32 and the float64 output hold exactly 0 and 1.
//
// Arithmetic.  d2 = |x|^2 + |f|^2 - 2 x.f, and |x|^2 is the same for every candidate of a query: the kernel minimises
//   e_i = |f_i|^2 - 2 x.f_i  =  d2 - |x|^2.
// Model load stores the fit rows as  -2 * code  (0, -2, -4: int8) and |f_i|^2 beside them; a 16 x 16 accumulator tile is
// INITIALISED with its columns' |f|^2 and v_mfma_i32_16x16x64_i8 adds the -2 x.f: the tile comes out of the matrix cores as e,
// and the only vector work per element is one compare and two selects.
// Layout (the structure of k_rbf_dec, svm/k_base_rbf.hip):
//  * one block = QB query haplotypes of one window (QB = 64, 32 or 16: the largest whose query tile fits the LDS), 4 waves;
//  * the queries' window bytes are gathered once into LDS, zero beyond the width; the fit rows sit in HBM as zero-padded rows of
//    kp = width rounded up to 64 bytes, n_fit rounded up to 128 rows; 16 aligned bytes of a row are one lane's B operand
//    (column = lane & 15, k-block = lane >> 4), 16 LDS bytes the A operand;
//  * per step of 128 fit rows wave v owns rows 32 v .. 32 v + 31 (two column tiles): per 64 SNPs it loads its two B operands
//    once and runs them against all QB / 16 query tiles (A operands from LDS), so one fit-row byte feeds QB MACs and one LDS
//    byte 32;
//  * every lane keeps, for each of its QB / 4 (query, column-of-16) slots, the running minimum (e, index) in registers.  A
//    lane meets its candidates in increasing index order, so `e < best` alone keeps the lowest index;
//  * once per query at the end: the 16 lanes and 4 waves that share a query reduce the 64-bit key  e * 2^32 + index  (signed;
//    index < 2^31 for any n_fit), which IS the tie rule; the winner's label is looked up and the one-hot rows are written.
//  * Padded fit rows (n_fit .. n_pad-1) never win: load gives exactly these indices |f|^2 = 2^30 (KNN_PAD_NORM), their bytes
//    are zero, so their e = 2^30, above any real row's e <= 4 * width.  (Unmasked they would hold e = 0 and beat or tie every
//    real row of an all-zero query.)
// No float64, no table, no distance ever leaves the registers, no scratch, no runtime-indexed array, plain vector stores.
// There is no training kernel: fitting a 1-NN classifier is storing the rows (gnomix_amd.train.train_knn_base).
#include "../gnx_internal.h"
#include "../gnx_window.h"

#include <cstring>

struct KnnWinDev {
  int32_t width, kp, n_fit, n_pad;  // SNPs; row pitch in bytes (width rounded up to 64); fit rows; rows rounded up to 128
  int64_t fit_off;                  // bytes: this window's rows [n_pad][kp], -2 * code, zero-padded
  int64_t row_off;                  // rows: |f|^2 and the label of (padded) row i are at row_off + i
};

struct KnnModel {
  const KnnWinDev* win = nullptr;
  const int8_t* fit = nullptr;
  const int32_t* yy = nullptr;
  const int32_t* lab = nullptr;
  int QB = 0;
  size_t lds = 0;
};

struct KnnLaunch {
  const int8_t* X;
  int64_t N, ldx, C, ctx, M;
  int32_t W, A, w_first;
  const KnnWinDev* win;
  const int8_t* fit;
  const int32_t* yy;
  const int32_t* lab;
  float* b32;
  double* b64;
};

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int32_t KNN_PAD_NORM = 1 << 30;
constexpr int KNN_STEP = 128;  // fit rows per step: 4 waves x 2 column tiles of 16

// red [QB][4] int64 | cls [QB] int32 | xq [QB][kp + 16] int8   (QB * 36 is a multiple of 16)
size_t knn_lds_bytes(int QB, int kp) { return (size_t)QB * 36 + (size_t)QB * (kp + 16); }

template <int QB>
__global__ __launch_bounds__(256) void k_knn_argmin(KnnLaunch L) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  constexpr int MTN = QB / 16;  // 16-query row tiles of the block
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int w = L.w_first + blockIdx.y;
  const KnnWinDev* wp = L.win + w;
  const int width = wp->width, kp = wp->kp, n_pad = wp->n_pad;
  const int xs = kp + 16;  // LDS row pitch of the query tile

  long long* red = reinterpret_cast<long long*>(lds);       // [QB][4]
  int32_t* cls = reinterpret_cast<int32_t*>(red + QB * 4);  // [QB]
  int8_t* xq = reinterpret_cast<int8_t*>(cls + QB);         // [QB][xs]

  const int64_t n0 = (int64_t)blockIdx.x * QB;

  // ---- the queries' window bytes over the reflect-padded coordinate, four per thread and store; rows past the batch repeat the
  //      last one (never written out) ----
  {
    const int64_t s = (int64_t)w * L.M;
    const int kq = kp / 4, total = QB * kq;
    for (int idx = t; idx < total; idx += 256) {
      const int q = idx / kq, k4 = (idx - q * kq) * 4;
      const int64_t n = (n0 + q < L.N) ? n0 + q : L.N - 1;
      const int8_t* row = L.X + n * L.ldx;
      uint32_t v = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if (k4 + b < width) v |= (uint32_t)(uint8_t)row[gnx_pad_src(s + k4 + b, L.C, L.ctx)] << (8 * b);
      *reinterpret_cast<uint32_t*>(xq + q * xs + k4) = v;
    }
  }
  __syncthreads();

  const int8_t* abase = xq + (lane & 15) * xs + (lane >> 4) * 16;
  const int8_t* fitw = L.fit + wp->fit_off;
  const int32_t* yyw = L.yy + wp->row_off;
  int bd[MTN][4], bi[MTN][4];
#pragma unroll
  for (int m = 0; m < MTN; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) { bd[m][r] = 0x7fffffff; bi[m][r] = 0; }

  for (int s0 = 0; s0 < n_pad; s0 += KNN_STEP) {
    const int r0 = s0 + wv * 32 + (lane & 15);  // this lane's fit row of the first column tile; the second is r0 + 16
    const int8_t* b0 = fitw + (size_t)r0 * kp + (lane >> 4) * 16;
    const int8_t* b1 = b0 + (size_t)16 * kp;
    const int y0 = yyw[r0], y1 = yyw[r0 + 16];
    v4i acc[MTN][2];
#pragma unroll
    for (int m = 0; m < MTN; ++m) { acc[m][0] = v4i{y0, y0, y0, y0}; acc[m][1] = v4i{y1, y1, y1, y1}; }
    for (int k0 = 0; k0 < kp; k0 += 64) {
      const v4i vb0 = *reinterpret_cast<const v4i*>(b0 + k0);
      const v4i vb1 = *reinterpret_cast<const v4i*>(b1 + k0);
#pragma unroll
      for (int m = 0; m < MTN; ++m) {
        const v4i a = *reinterpret_cast<const v4i*>(abase + m * 16 * xs + k0);
        acc[m][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, vb0, acc[m][0], 0, 0, 0);
        acc[m][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, vb1, acc[m][1], 0, 0, 0);
      }
    }
    // int32 16x16 C/D layout: column (fit row) = lane & 15, row (query) = 4 * (lane >> 4) + reg.  Indices rise with u, then s0.
#pragma unroll
    for (int m = 0; m < MTN; ++m)
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int e = acc[m][u][r];
          const bool lt = e < bd[m][r];
          bd[m][r] = lt ? e : bd[m][r];
          bi[m][r] = lt ? r0 + 16 * u : bi[m][r];
        }
  }

  // ---- once per query: min of (e, index) over the 16 lanes of a row group, then over the 4 waves ----
#pragma unroll
  for (int m = 0; m < MTN; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      long long key = (long long)bd[m][r] * 4294967296LL + (long long)bi[m][r];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        const long long other = __shfl_xor(key, o, 64);
        key = other < key ? other : key;
      }
      if ((lane & 15) == 0) red[(m * 16 + 4 * (lane >> 4) + r) * 4 + wv] = key;
    }
  __syncthreads();
  if (t < QB) {
    long long key = red[t * 4];
#pragma unroll
    for (int v = 1; v < 4; ++v) key = red[t * 4 + v] < key ? red[t * 4 + v] : key;
    cls[t] = L.lab[wp->row_off + (int64_t)(key & 0xffffffffLL)];
  }
  __syncthreads();
  const int A = L.A;
  for (int i = t; i < QB * A; i += 256) {
    const int q = i / A, c = i - q * A;
    if (n0 + q < L.N) {
      const size_t o = ((size_t)(n0 + q) * L.W + w) * A + c;
      const bool hit = cls[q] == c;
      if (L.b32) L.b32[o] = hit ? 1.0f : 0.0f;
      if (L.b64) L.b64[o] = hit ? 1.0 : 0.0;
    }
  }
}

template <int QB>
hipError_t launch_knn(const KnnLaunch& L, size_t lds, hipStream_t s) {
  GNX_LDS_OPTIN(lds, k_knn_argmin<QB>);
  for (int w0 = 0; w0 < L.W; w0 += 32768) {
    KnnLaunch Lw = L;
    Lw.w_first = w0;
    const dim3 grid((unsigned)((L.N + QB - 1) / QB), (unsigned)std::min(32768, L.W - w0));
    hipLaunchKernelGGL(k_knn_argmin<QB>, grid, dim3(256), lds, s, Lw);
  }
  return hipGetLastError();
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// model preparation: fit rows as -2 * code at the kernel's pitch, |f|^2 (2^30 for padded rows), labels
// ------------------------------------------------------------------------------------------------
int gnx_build_knn(gnx_model* m, const gnx_model_desc* d) {
  gnx_ctx* ctx = m->ctx;
  const int A = d->A;
  const int64_t C = d->C, M = d->M, W = C / M, rem = C - M * W, M_ = M + 2 * d->ctx;
  if (!d->knn) return gnx_fail(ctx, GNX_EINVAL, "knn base: knn array is NULL");
  if (M_ + rem > GNX_RBF_MAX_WIDTH) return gnx_fail(ctx, GNX_EUNSUPPORTED, "knn base: windows wider than GNX_RBF_MAX_WIDTH SNPs");
  std::vector<KnnWinDev> wins((size_t)W);
  int64_t bytes = 0, rows = 0;
  int max_kp = 0;
  for (int64_t i = 0; i < W; ++i) {
    const gnx_knn_window& kw = d->knn[i];
    const std::string wn = "knn base: window " + std::to_string(i) + ": ";
    const int64_t width = (i == W - 1) ? M_ + rem : M_;
    if (kw.width != width) return gnx_fail(ctx, GNX_EINVAL, wn + "knn[i].width != window width (M+2ctx, +rem for the last)");
    if (kw.n_fit < 1) return gnx_fail(ctx, GNX_EINVAL, wn + "n_fit < 1");
    if (kw.n_fit > (1 << 30)) return gnx_fail(ctx, GNX_EUNSUPPORTED, wn + "more than 2^30 fit rows");
    if (!kw.xfit || !kw.y) return gnx_fail(ctx, GNX_EINVAL, wn + "xfit / y is NULL");
    KnnWinDev& wd = wins[(size_t)i];
    wd.width = (int32_t)width;
    wd.kp = (int32_t)((width + 63) / 64 * 64);
    wd.n_fit = kw.n_fit;
    wd.n_pad = (int32_t)(((int64_t)kw.n_fit + KNN_STEP - 1) / KNN_STEP * KNN_STEP);
    wd.fit_off = bytes;
    wd.row_off = rows;
    bytes += (int64_t)wd.n_pad * wd.kp;
    rows += wd.n_pad;
    max_kp = std::max(max_kp, wd.kp);
  }
  std::vector<int8_t> fit((size_t)bytes, 0);
  std::vector<int32_t> yy((size_t)rows, KNN_PAD_NORM), lab((size_t)rows, 0);
  for (int64_t i = 0; i < W; ++i) {
    const gnx_knn_window& kw = d->knn[i];
    const KnnWinDev& wd = wins[(size_t)i];
    const std::string wn = "knn base: window " + std::to_string(i) + ": ";
    for (int32_t k = 0; k < kw.n_fit; ++k) {
      const int8_t* row = kw.xfit + (size_t)k * wd.width;
      int8_t* dst = fit.data() + wd.fit_off + (size_t)k * wd.kp;
      int32_t s2 = 0;
      for (int32_t t = 0; t < wd.width; ++t) {
        const int8_t v = row[t];
        if (v < 0 || v > 2) return gnx_fail(ctx, GNX_EINVAL, wn + "fit row " + std::to_string(k) + " holds " + std::to_string((int)v) +
                                                            " at SNP " + std::to_string(t) + " (codes must be 0..2)");
        dst[t] = (int8_t)(-2 * v);
        s2 += (int32_t)v * v;
      }
      const int32_t y = kw.y[k];
      if (y < 0 || y >= A) return gnx_fail(ctx, GNX_EINVAL, wn + "label " + std::to_string(y) + " of fit row " + std::to_string(k) +
                                                       " is outside [0, A)");
      yy[(size_t)wd.row_off + k] = s2;
      lab[(size_t)wd.row_off + k] = y;
    }
  }
  auto knn = std::make_shared<KnnModel>();
  for (int QB : {64, 32, 16})
    if (knn_lds_bytes(QB, max_kp) <= (size_t)160 * 1024) { knn->QB = QB; break; }
  if (!knn->QB) return gnx_fail(ctx, GNX_EUNSUPPORTED, "knn base: window too wide for the LDS query tile");
  knn->lds = knn_lds_bytes(knn->QB, max_kp);
  int rc;
  if ((rc = gnx_dev_upload(m, wins, &knn->win)) != GNX_OK) return rc;
  if ((rc = gnx_dev_upload(m, fit, &knn->fit, 64)) != GNX_OK) return rc;
  if ((rc = gnx_dev_upload(m, yy, &knn->yy)) != GNX_OK) return rc;
  if ((rc = gnx_dev_upload(m, lab, &knn->lab)) != GNX_OK) return rc;
  m->knn = knn;
  return GNX_OK;
}

int gnx_base_predict_knn(gnx_model* m, const int8_t* dX, int64_t N, int64_t ldx, float* d_b32, double* d_b64) {
  gnx_ctx* ctx = m->ctx;
  if (!m->knn) return gnx_fail(ctx, GNX_ESTATE, "knn base: model holds no prepared windows");
  const KnnModel& K = *m->knn;
  KnnLaunch L{};
  L.X = dX; L.N = N; L.ldx = ldx; L.C = m->info.C; L.ctx = m->info.ctx; L.M = m->info.M;
  L.W = (int32_t)m->info.W; L.A = m->info.A;
  L.win = K.win; L.fit = K.fit; L.yy = K.yy; L.lab = K.lab;
  L.b32 = d_b32; L.b64 = d_b64;
  switch (K.QB) {
    case 64: HIPCHK(ctx, launch_knn<64>(L, K.lds, ctx->stream)); break;
    case 32: HIPCHK(ctx, launch_knn<32>(L, K.lds, ctx->stream)); break;
    default: HIPCHK(ctx, launch_knn<16>(L, K.lds, ctx->stream)); break;
  }
  return GNX_OK;
}
